"""fpga-mpeg2-encoder_amd — MI355X-native MPEG-2 I/P encoder, drop-in for RTL/mpeg2encoder.v.

This package is plumbing: it loads libm2v_mi355x.so (hand-written HIP for gfx950 behind the
C-ABI of include/m2v_mi355x.h) through ctypes and mirrors the module's port contract
(parameters XL/YL/VECTOR_LEVEL/Q_LEVEL; beats in; 32-byte stream words out).  There is no CPU
fallback: without the built library or without a GPU every entry point raises.
"""
import contextlib
import ctypes
import functools
import os
import sys
import threading

import numpy as np

from . import build as _build
from . import synth  # noqa: F401  (seeded synthetic clips, numpy only)
from . import parallel  # noqa: F401  (multi-GPU: independent sequences, macroblock-row strips)
from . import container  # noqa: F401  (CPU-side conveniences: stream scan, MPEG-PS / TS multiplexers)
from . import decoder  # noqa: F401  (analysis tool: MPEG-2 ES decoder written from ISO/IEC 13818-2, CPU, not on the encode path)

_HERE = os.path.dirname(os.path.abspath(__file__))
# M2V_LIB: development hook for same-box A/B timing of two builds (tools/ab.sh); never set otherwise
LIB_PATH = os.environ.get("M2V_LIB") or os.path.join(_HERE, "libm2v_mi355x.so")
# the -DM2V_DEBUG build (level dump, "keep_recon", "inject_strip_failure"): stage-level parity tests and profiling scripts only
LIB_DBG_PATH = os.environ.get("M2V_LIB_DBG") or os.path.join(_HERE, "libm2v_mi355x_dbg.so")

_libs = {}

EXPORTS = [
    "m2v_version", "m2v_create", "m2v_destroy", "m2v_reset", "m2v_push_beats", "m2v_push_packed", "m2v_push_frames", "m2v_push_frames_pull",
    "m2v_sequence_stop", "m2v_busy", "m2v_pull", "m2v_geometry", "m2v_encode_resident", "m2v_encode_resident_begin",
    "m2v_encode_resident_end", "m2v_set_option",
    "m2v_kernel_stats", "m2v_debug_read", "m2v_last_error", "m2v_debug_table",
    "m2v_strip_begin", "m2v_strip_info", "m2v_strip_step", "m2v_strip_step_edges", "m2v_strip_step_interior", "m2v_strip_halo_in", "m2v_strip_finish", "m2v_strip_assemble",
    "m2v_strip_finish_async", "m2v_strip_offsets", "m2v_strip_encode", "m2v_strip_stats",
    "m2v_comm_unique_id", "m2v_comm_init_rccl", "m2v_comm_init_local", "m2v_comm_init_solo", "m2v_comm_destroy", "m2v_comm_last_error", "m2v_comm_selftest",
    "m2v_comm_init_solo_rccl", "m2v_comm_selftest_captured", "m2v_strip_graph_stats",
    "m2v_comm_init_callbacks", "m2v_comm_init_peer", "m2v_comm_peer_export", "m2v_comm_peer_connect", "m2v_comm_peer_connect_all",
    "m2v_comm_peer_stats", "m2v_comm_kind", "m2v_strip_last_form", "m2v_upload_wait", "m2v_device_pci_bus_id",
    "m2v_strip_encode_begin", "m2v_strip_encode_end",
    "m2v_rgb_matrix", "m2v_push_rgb", "m2v_push_rgb_pull", "m2v_encode_resident_rgb", "m2v_encode_resident_rgb_begin",
    "m2v_set_frame_size", "m2v_fit_size", "m2v_picture_stats",
    "m2v_set_gop_levels", "m2v_gop_report",
    "m2v_set_gop_starts", "m2v_gop_layout", "m2v_scene_report",
    "m2v_set_recon_out",
    "m2v_stream_desc_module", "m2v_set_stream_desc", "m2v_frame_rate_code", "m2v_time_code",
    "m2v_set_sequences", "m2v_sequence_report",
    "m2v_mux_bound", "m2v_set_mux_out", "m2v_mux_report", "m2v_mux_device", "m2v_mux_scan_tile",
    "m2v_set_source_size", "m2v_scale_taps",
    "m2v_demux_bound", "m2v_demux_device", "m2v_demux_report", "m2v_demux_scan_tile",
    "m2v_decode_streams_device", "m2v_decode_streams_report", "m2v_decode_streams_main_device", "m2v_decode_streams_main_ex_device",
    "m2v_deinterlace_device", "m2v_deinterlace_bound", "m2v_deinterlace_tile",
]

# the 4:2:0 entry points (kept apart: tests/test_abi.py matches EXPORTS against names of letters and underscores only)
EXPORTS_420 = ["m2v_push_frames420", "m2v_push_frames420_pull", "m2v_encode_resident420", "m2v_encode_resident420_begin"]
LAYOUTS_420 = {"i420": 0, "yv12": 1, "nv12": 2, "nv21": 3}          # M2V_420_*

# RGB input (include/m2v_mi355x.h).  M2V_RGB_* layouts: name -> code; bytes per pixel and where R, G, B sit (rgbp: which plane)
LAYOUTS_RGB = {"rgb24": 0, "bgr24": 1, "rgbx": 2, "bgrx": 3, "xrgb": 4, "xbgr": 5, "rgbp": 6}
_RGB_FORM = {0: (3, (0, 1, 2)), 1: (3, (2, 1, 0)), 2: (4, (0, 1, 2)), 3: (4, (2, 1, 0)), 4: (4, (1, 2, 3)), 5: (4, (3, 2, 1)), 6: (3, (0, 1, 2))}
# the matrices: name -> (code, T row by row (Y, U, V x R, G, B; scale 2^14), luma offset).  Typed out here, independent of the
# library's table (m2v_rgb_matrix); tests/test_input_rgb.py holds the two against each other and against the derivation.
MATRICES_RGB = {
    "bt601": (0, (4207, 8260, 1604, -2428, -4768, 7196, 7196, -6026, -1170), 16),
    "bt709": (1, (2991, 10064, 1016, -1649, -5547, 7196, 7196, -6536, -660), 16),
    "bt601f": (2, (4899, 9617, 1868, -2765, -5427, 8192, 8192, -6860, -1332), 0),
    "bt709f": (3, (3483, 11718, 1183, -1877, -6315, 8192, 8192, -7441, -751), 0),
}

PEER_DESC_BYTES = 128          # M2V_PEER_DESC_BYTES


class PictureStat(ctypes.Structure):
    """m2v_picture_stat (include/m2v_mi355x.h): one picture's record of option "stats", 64 bytes"""
    _fields_ = [("frame", ctypes.c_uint32), ("coding_type", ctypes.c_uint32), ("sse", ctypes.c_uint64 * 3), ("mb_bits", ctypes.c_uint64),
                ("intra_mbs", ctypes.c_uint32), ("inter_mbs", ctypes.c_uint32), ("coded_blocks", ctypes.c_uint32),
                ("mv_abs_x", ctypes.c_uint32), ("mv_abs_y", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


# the same record as a numpy structured dtype (Mpeg2Encoder.picture_stats)
PICTURE_STAT_DTYPE = np.dtype([("frame", "<u4"), ("coding_type", "<u4"), ("sse", "<u8", (3,)), ("mb_bits", "<u8"), ("intra_mbs", "<u4"),
                               ("inter_mbs", "<u4"), ("coded_blocks", "<u4"), ("mv_abs_x", "<u4"), ("mv_abs_y", "<u4"), ("reserved", "<u4")])


class GopStat(ctypes.Structure):
    """m2v_gop_stat (include/m2v_mi355x.h): one GOP's record of option "gop_bytes_max", 32 bytes"""
    _fields_ = [("gop", ctypes.c_uint32), ("first_frame", ctypes.c_uint32), ("frames", ctypes.c_uint32), ("level", ctypes.c_uint32),
                ("bytes", ctypes.c_uint64), ("tries", ctypes.c_uint32), ("over", ctypes.c_uint32)]


# the same record as a numpy structured dtype (Mpeg2Encoder.gop_report)
GOP_STAT_DTYPE = np.dtype([("gop", "<u4"), ("first_frame", "<u4"), ("frames", "<u4"), ("level", "<u4"), ("bytes", "<u8"), ("tries", "<u4"),
                           ("over", "<u4")])


class SceneStat(ctypes.Structure):
    """m2v_scene_stat (include/m2v_mi355x.h): one picture's record of m2v_set_gop_starts / option "scene_cut", 16 bytes"""
    _fields_ = [("frame", ctypes.c_uint32), ("flags", ctypes.c_uint32), ("diff", ctypes.c_uint64)]


# the same record as a numpy structured dtype (Mpeg2Encoder.scene_report)
SCENE_STAT_DTYPE = np.dtype([("frame", "<u4"), ("flags", "<u4"), ("diff", "<u8")])
GOP_FIRST, GOP_CADENCE, GOP_LIST, GOP_CUT = 1, 2, 4, 8           # M2V_GOP_*


class SequenceStat(ctypes.Structure):
    """m2v_sequence_stat (include/m2v_mi355x.h): one clip's record of a batch (m2v_set_sequences), 32 bytes"""
    _fields_ = [("offset", ctypes.c_uint64), ("bytes", ctypes.c_uint64), ("first_frame", ctypes.c_uint32), ("frames", ctypes.c_uint32),
                ("gops", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


# the same record as a numpy structured dtype (Mpeg2Encoder.sequence_report)
SEQUENCE_STAT_DTYPE = np.dtype([("offset", "<u8"), ("bytes", "<u8"), ("first_frame", "<u4"), ("frames", "<u4"), ("gops", "<u4"),
                                ("reserved", "<u4")])


# m2v_mux_stat (include/m2v_mi355x.h): one container's record of m2v_set_mux_out / m2v_mux_device, 40 bytes (Mpeg2Encoder.mux_report)
MUX_STAT_DTYPE = np.dtype([("es_offset", "<u8"), ("es_bytes", "<u8"), ("out_offset", "<u8"), ("out_bytes", "<u8"), ("pictures", "<u4"),
                           ("status", "<i4")])
MUX_KINDS = {"ts": 1, "ps": 2}                                   # M2V_MUX_*
MUX_OK, MUX_SYNTAX, MUX_OVERFLOW = 0, -2, -3


# m2v_decode_stat (include/m2v_mi355x.h): the record of m2v_decode_device, 72 bytes (Mpeg2Encoder.decode_report)
DECODE_STAT_DTYPE = np.dtype([("es_bytes", "<u8"), ("out_bytes", "<u8"), ("frame_bytes", "<u8"), ("err_offset", "<u8"), ("pictures", "<u4"),
                              ("gops", "<u4"), ("width", "<u4"), ("height", "<u4"), ("repeated_headers", "<u4"), ("chains", "<u4"),
                              ("status", "<i4"), ("reserved", "<u4", (3,))])
# m2v_decode_stream_stat: one stream's record of m2v_decode_streams_device, 88 bytes (Mpeg2Encoder.decode_streams_report)
DECODE_STREAM_STAT_DTYPE = np.dtype([("es_offset", "<u8"), ("out_offset", "<u8"), ("rec", DECODE_STAT_DTYPE)])
# m2v_decode_join: the join record of the last decode_device, 32 bytes (Mpeg2Encoder.decode_join_report)
DECODE_JOIN_DTYPE = np.dtype([("join_offset", "<u8"), ("tail_offset", "<u8"), ("dropped_leading", "<u4"), ("dropped_trailing", "<u4"), ("reserved", "<u4", (2,))])
# m2v_decode_conceal: the concealment report of the last decode_device, 32 bytes (Mpeg2Encoder.decode_conceal_report)
DECODE_CONCEAL_DTYPE = np.dtype([("first_offset", "<u8"), ("bad_slices", "<u4"), ("concealed_rows", "<u4"), ("grey_rows", "<u4"), ("damaged_pictures", "<u4"),
                                 ("reserved", "<u4", (2,))])
DEC_JOINS = {"head": 1, "tail": 2, "both": 3}                    # M2V_JOIN_*: option "decode_join"
DEC_MODES = {"iso": 0, "module": 1}                              # M2V_DEC_*
DEC_SYNTAXES = {"module": 0, "main": 1}                          # M2V_SYNTAX_*: option "decode_syntax"
DECS_B_PICTURES, DECS_INTERLACED = 1, 2                          # M2V_DECS_*: the flags of m2v_decode_streams_main_device
DECS_EXTENDED, DECS_MB_TOOLS = 4, 8                              # ... and the two further ones of m2v_decode_streams_main_ex_device
DEC_OK, DEC_SYNTAX, DEC_OVERFLOW = 0, -2, -3
DEC_STATUS = {0: "M2V_DEC_OK", -2: "M2V_DEC_SYNTAX", -3: "M2V_DEC_OVERFLOW"}


# m2v_demux_stat (include/m2v_mi355x.h): one container's record of m2v_demux_device, 64 bytes (Mpeg2Encoder.demux_report), and
# m2v_demux_stamp: one PES packet of a demultiplexed stream, 32 bytes (pts / dts = DEMUX_ABSENT when the header carries none)
DEMUX_STAT_DTYPE = np.dtype([("src_offset", "<u8"), ("src_bytes", "<u8"), ("out_offset", "<u8"), ("out_bytes", "<u8"), ("err_offset", "<u8"),
                             ("pes_packets", "<u4"), ("packets", "<u4"), ("discontinuities", "<u4"), ("skipped", "<u4"), ("stream", "<u4"),
                             ("status", "<i4")])
DEMUX_STAMP_DTYPE = np.dtype([("es_offset", "<u8"), ("pts", "<u8"), ("dts", "<u8"), ("src_offset", "<u8")])
DEMUX_OK, DEMUX_SYNTAX, DEMUX_OVERFLOW, DEMUX_NOSTREAM = 0, -2, -3, -4
DEMUX_STATUS = {0: "M2V_DEMUX_OK", -2: "M2V_DEMUX_SYNTAX", -3: "M2V_DEMUX_OVERFLOW", -4: "M2V_DEMUX_NOSTREAM"}
DEMUX_ABSENT = 0xFFFFFFFFFFFFFFFF


def demux_scan_tile():
    """m2v_demux_scan_tile: the bytes of a transport stream after which the device demultiplexer hands over to another workgroup"""
    return int(lib().m2v_demux_scan_tile())


def demux_bound(sizes):
    """m2v_demux_bound: bytes that always suffice for the elementary streams of containers of these sizes"""
    a = (ctypes.c_uint64 * max(len(sizes), 1))(*[int(b) for b in sizes])
    return int(lib().m2v_demux_bound(a, len(sizes)))


def decode_scan_tile():
    """m2v_decode_scan_tile: the byte span after which the device decoder's start-code scan hands over to another workgroup"""
    return int(lib().m2v_decode_scan_tile())


def frames_of_stream(frames, rec):
    """the [pictures, frame_bytes] view of one stream's frames in what decode_streams returned; rec: its record.  Empty where the
    stream's status is not DEC_OK (out_bytes 0)"""
    r = rec["rec"]
    n, fb = (int(r["pictures"]), int(r["frame_bytes"])) if int(r["out_bytes"]) else (0, int(r["frame_bytes"]))
    at = int(rec["out_offset"])
    return frames[at:at + n * fb].reshape(n, fb)


def _mux_kind(kind):
    if isinstance(kind, str):
        if kind not in MUX_KINDS:
            raise ValueError("unknown container %r (one of %s)" % (kind, ", ".join(MUX_KINDS)))
        return MUX_KINDS[kind]
    return int(kind)


def mux_bound(kind, es_bytes, pictures):
    """m2v_mux_bound: bytes that always suffice for the container of a stream of es_bytes bytes and `pictures` pictures"""
    return int(lib().m2v_mux_bound(_mux_kind(kind), int(es_bytes), int(pictures)))


def mux_scan_tile():
    """m2v_mux_scan_tile: the byte span after which the device muxer's start-code scan hands over to another workgroup"""
    return int(lib().m2v_mux_scan_tile())


def check_sequences(lengths, nframes):
    """the rule of m2v_set_sequences for a call of nframes frames, as plain arithmetic: the list of ints, or ValueError for an entry
    below 1 or a sum that is not nframes"""
    ln = [int(v) for v in lengths]
    if any(v < 1 or v > 0xFFFFFFFF for v in ln):
        raise ValueError("sequences: every entry is 1 .. 2^32 - 1 frames, got %r" % (ln,))
    if sum(ln) != int(nframes):
        raise ValueError("sequences: the entries add up to %d, the call has %d frames" % (sum(ln), int(nframes)))
    return ln


class StreamDesc(ctypes.Structure):
    """m2v_stream_desc (include/m2v_mi355x.h): what the stream says about itself, 48 bytes"""
    _fields_ = [(k, ctypes.c_uint32) for k in ("frame_rate_code", "aspect_ratio_information", "bit_rate_400", "vbv_buffer_size_16k",
                                               "video_format", "colour_primaries", "transfer_characteristics", "matrix_coefficients",
                                               "display_width", "display_height", "repeat_headers", "reserved")]

    def __repr__(self):
        return "StreamDesc(%s)" % ", ".join("%s=%d" % (k, getattr(self, k)) for k, _ in self._fields_)


FRAME_RATES = {1: (24000, 1001), 2: (24, 1), 3: (25, 1), 4: (30000, 1001), 5: (30, 1), 6: (50, 1), 7: (60000, 1001), 8: (60, 1)}   # table 6-4
ASPECTS = {"1:1": 1, "4:3": 2, "16:9": 3, "2.21:1": 4}                                                                             # table 6-3
COLOURS = {"bt709": (1, 1, 1), "bt601": (5, 5, 5)}              # colour_primaries, transfer_characteristics, matrix_coefficients


def frame_rate_code(num, den=1):
    """m2v_frame_rate_code: 1..8 for a rational equal to an entry of table 6-4, ValueError otherwise.  Plain arithmetic, no GPU."""
    r = lib().m2v_frame_rate_code(int(num), int(den)) if 0 <= int(num) <= 0xFFFFFFFF and 0 <= int(den) <= 0xFFFFFFFF else -1
    if r < 0:
        raise ValueError("frame_rate_code: %r/%r is not a frame rate of ISO/IEC 13818-2 table 6-4" % (num, den))
    return r


def time_code(n, code=2):
    """m2v_time_code: the four bytes behind 00 00 01 B8 for a GOP that starts at frame n, at frame_rate_code `code`.  No GPU."""
    out = (ctypes.c_uint8 * 4)()
    if lib().m2v_time_code(int(code), int(n) & 0xFFFFFFFF, out) < 0:
        raise ValueError("time_code: frame_rate_code %r is not 1..8" % (code,))
    return bytes(out)


def stream_desc(fps=None, aspect=None, bit_rate=None, vbv_bits=None, video_format=None, colour=None, display=None, repeat_headers=False):
    """A StreamDesc for Mpeg2Encoder.set_stream_desc: the module's values (m2v_stream_desc_module) with the given ones replaced.
    fps: a (num, den) pair equal to an entry of table 6-4, or a number within 1e-3 of one;  aspect: "1:1", "4:3", "16:9" or "2.21:1";
    bit_rate: bit/s, rounded up to units of 400;  vbv_bits: bits, rounded up to units of 16384;  video_format: 0..5;
    colour: "bt709" (1 / 1 / 1), "bt601" (5 / 5 / 5) or a triple of codes, taken as is;  display: (width, height);
    repeat_headers: the sequence headers again in front of every GOP after the first.  ValueError for what names no value; the ranges
    are m2v_set_stream_desc's to check."""
    d = StreamDesc()
    lib().m2v_stream_desc_module(ctypes.byref(d))
    if fps is not None:
        if isinstance(fps, (tuple, list)):
            d.frame_rate_code = frame_rate_code(*fps)
        else:
            near = [c for c, (n, m) in FRAME_RATES.items() if abs(float(fps) - n / m) <= 1e-3]
            if not near:
                raise ValueError("stream_desc: fps %r is not within 1e-3 of a frame rate of table 6-4" % (fps,))
            d.frame_rate_code = near[0]
    if aspect is not None:
        if aspect not in ASPECTS:
            raise ValueError("stream_desc: unknown aspect %r" % (aspect,))
        d.aspect_ratio_information = ASPECTS[aspect]
    if bit_rate is not None:
        d.bit_rate_400 = -(-int(bit_rate) // 400)
    if vbv_bits is not None:
        d.vbv_buffer_size_16k = -(-int(vbv_bits) // 16384)
    if video_format is not None:
        d.video_format = int(video_format)
    if colour is not None:
        if isinstance(colour, str) and colour not in COLOURS:
            raise ValueError("stream_desc: unknown colour %r" % (colour,))
        d.colour_primaries, d.transfer_characteristics, d.matrix_coefficients = COLOURS[colour] if isinstance(colour, str) else colour
    if display is not None:
        d.display_width, d.display_height = display
    d.repeat_headers = 1 if repeat_headers else 0
    return d


def _uint_list(values, ctype, error):
    """`values` (None: none) for the ABI: (the list of ints, a ctypes array of ctype - None for an empty list, which clears a setting);
    raises `error` for an entry that does not fit ctype"""
    v = [] if values is None else [int(x) for x in values]
    if any(x < 0 or x >> (8 * ctypes.sizeof(ctype)) for x in v):
        raise error
    return v, (ctype * len(v))(*v) if v else None


def gop_layout(pframes_count, starts, nframes):
    """m2v_gop_layout: (the M2V_GOP_* reasons of each of nframes frames as a uint8 array - non-zero where a GOP starts -, the number
    of GOPs) for pframes_count and the list `starts` (strictly ascending, ValueError otherwise).  Plain arithmetic, no GPU."""
    st, buf = _uint_list(starts, ctypes.c_uint32, ValueError("gop_layout: a frame number is 0 .. 2^32 - 1"))
    flags = np.zeros(int(nframes), np.uint8)
    n = lib().m2v_gop_layout(int(pframes_count), buf, len(st), int(nframes), flags.ctypes.data if nframes else None)
    if n < 0:
        raise ValueError("gop_layout: the list must be strictly ascending")
    return flags, int(n)


def psnr_from_sse(sse, samples):
    """10 log10(255^2 * samples / sse) in dB, inf where sse == 0: the PSNR of a plane (or of several: add their sse and their samples)
    from a record's exact sum of squared errors.  Scalars or arrays."""
    sse = np.asarray(sse, np.float64)
    with np.errstate(divide="ignore"):
        out = 10.0 * np.log10(255.0 * 255.0 * np.asarray(samples, np.float64) / sse)
    return float(out) if out.ndim == 0 else out


class CommCallbacks(ctypes.Structure):
    """m2v_comm_callbacks (include/m2v_mi355x.h): the exchange supplied by the caller"""
    HALO = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                            ctypes.c_size_t, ctypes.c_void_p)
    ALLGATHER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p)
    GATHER = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t),
                              ctypes.POINTER(ctypes.c_void_p), ctypes.c_void_p)
    _fields_ = [("halo", HALO), ("allgather_u64", ALLGATHER), ("gather", GATHER), ("user", ctypes.c_void_p)]


class M2VError(RuntimeError):
    pass


def lib(debug=False):
    """The C-ABI shared library; raises if it has not been built (no silent fallback).
    debug=True: the -DM2V_DEBUG build of the same sources (tests and profiling only)."""
    path = LIB_DBG_PATH if debug else LIB_PATH
    if path not in _libs:
        if not os.path.exists(path):
            raise M2VError("%s is missing: run __graft_entry__.build() "
                           "(hipcc, gfx950); there is no CPU fallback" % os.path.basename(path))
        # One process must hold ONE HIP runtime.  PyTorch-ROCm (used here only for device memory and
        # streams) bundles its own libamdhip64; importing it first makes the loader resolve this
        # library's libamdhip64.so.7 dependency to the copy torch already mapped.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        L = ctypes.CDLL(path)
        vp, sz, u32, ci = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32, ctypes.c_int
        L.m2v_version.restype = ctypes.c_char_p
        L.m2v_create.restype = vp
        L.m2v_create.argtypes = [ci, ci, ci, ci, ci, ctypes.POINTER(ci)]
        L.m2v_destroy.argtypes = [vp]
        L.m2v_reset.argtypes = [vp]
        L.m2v_push_beats.argtypes = [vp, u32, u32, u32, vp, vp, vp, sz, ci]
        L.m2v_push_packed.argtypes = [vp, u32, u32, u32, vp, sz, ci, ci]
        L.m2v_push_frames.argtypes = [vp, u32, u32, u32, vp, sz]
        L.m2v_sequence_stop.argtypes = [vp]
        L.m2v_busy.argtypes = [vp]
        L.m2v_pull.restype = ctypes.c_longlong
        L.m2v_pull.argtypes = [vp, vp, sz, ctypes.POINTER(ci)]
        L.m2v_geometry.argtypes = [vp, u32, u32, ctypes.POINTER(ci), ctypes.POINTER(ci)]
        L.m2v_encode_resident.argtypes = [vp, u32, u32, u32, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
        L.m2v_encode_resident_begin.argtypes = [vp, u32, u32, u32, vp, sz, vp, sz, vp]
        L.m2v_encode_resident_end.argtypes = [vp, ctypes.POINTER(sz)]
        L.m2v_set_option.argtypes = [vp, ctypes.c_char_p, ctypes.c_longlong]
        L.m2v_kernel_stats.argtypes = [vp, ci, ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double)]
        L.m2v_debug_read.restype = ctypes.c_longlong
        L.m2v_debug_read.argtypes = [vp, ci, vp, sz]
        L.m2v_last_error.restype = ctypes.c_char_p
        L.m2v_last_error.argtypes = [vp]
        L.m2v_debug_table.argtypes = [ci, ci, ci]
        L.m2v_strip_begin.argtypes = [vp, u32, u32, u32, vp, sz, ci, ci, vp]
        L.m2v_strip_info.argtypes = [vp, ctypes.POINTER(ci), ctypes.POINTER(sz)]
        L.m2v_strip_step.argtypes = [vp, ci, vp, vp]
        L.m2v_strip_step_edges.argtypes = [vp, ci, vp, vp]
        L.m2v_strip_step_interior.argtypes = [vp, ci]
        L.m2v_strip_halo_in.argtypes = [vp, ci, vp, vp]
        L.m2v_strip_finish.argtypes = [vp, vp, sz, vp]
        L.m2v_strip_assemble.argtypes = [vp, u32, u32, u32, sz, ci, vp, vp, vp, sz, ctypes.POINTER(sz), vp]
        try:
            L.m2v_strip_finish_async.argtypes = [vp, vp, sz]
            L.m2v_strip_offsets.argtypes = [vp, vp]
            L.m2v_strip_encode.argtypes = [vp, vp, ci, ci, ci, u32, u32, u32, vp, sz, vp, sz, ctypes.POINTER(sz), vp]
            dp = ctypes.POINTER(ctypes.c_double)
            L.m2v_strip_stats.argtypes = [vp, dp, dp, dp, dp, dp]
            L.m2v_comm_init_solo.restype = vp
            L.m2v_comm_init_solo.argtypes = [ci, ctypes.POINTER(ci)]
            L.m2v_comm_unique_id.argtypes = [vp, sz]
            L.m2v_comm_init_rccl.restype = vp
            L.m2v_comm_init_rccl.argtypes = [vp, ci, ci, ci, ctypes.POINTER(ci)]
            L.m2v_comm_init_local.restype = vp
            L.m2v_comm_init_local.argtypes = [ci, ctypes.POINTER(ci)]
            L.m2v_comm_destroy.argtypes = [vp]
            L.m2v_comm_last_error.restype = ctypes.c_char_p
            L.m2v_comm_selftest.argtypes = [vp, ci, vp, vp, sz, vp]
            L.m2v_comm_init_solo_rccl.restype = vp
            L.m2v_comm_init_solo_rccl.argtypes = [ci, ctypes.POINTER(ci)]
            L.m2v_comm_selftest_captured.argtypes = [vp, ci, vp, vp, sz, vp, ci]
            ip = ctypes.POINTER(ci)
            L.m2v_strip_graph_stats.argtypes = [vp, ip, ip, ip]
            L.m2v_comm_init_callbacks.restype = vp
            L.m2v_comm_init_callbacks.argtypes = [ci, ctypes.POINTER(CommCallbacks), ip]
            L.m2v_comm_init_peer.restype = vp
            L.m2v_comm_init_peer.argtypes = [vp, ci, ci, sz, ip]
            L.m2v_comm_peer_export.argtypes = [vp, vp, sz]
            L.m2v_comm_peer_connect.argtypes = [vp, vp, vp]
            L.m2v_comm_peer_connect_all.argtypes = [vp]
            ullp = ctypes.POINTER(ctypes.c_ulonglong)
            L.m2v_comm_peer_stats.argtypes = [vp, ullp, ullp]
            L.m2v_comm_kind.restype = ctypes.c_char_p
            L.m2v_comm_kind.argtypes = [vp]
            L.m2v_strip_last_form.argtypes = [vp]
            L.m2v_upload_wait.argtypes = [vp]
            L.m2v_push_frames_pull.restype = ctypes.c_longlong
            L.m2v_push_frames_pull.argtypes = [vp, u32, u32, u32, vp, sz, vp, sz, ctypes.POINTER(ci)]
            L.m2v_device_pci_bus_id.argtypes = [ci, ctypes.c_char_p, sz]
            L.m2v_strip_encode_begin.argtypes = [vp, vp, ci, ci, ci, u32, u32, u32, vp, sz, vp, sz, vp]
            L.m2v_strip_encode_end.argtypes = [vp, ctypes.POINTER(sz)]
            L.m2v_push_frames420.argtypes = [vp, u32, u32, u32, vp, sz, ci]
            L.m2v_push_frames420_pull.restype = ctypes.c_longlong
            L.m2v_push_frames420_pull.argtypes = [vp, u32, u32, u32, vp, sz, ci, vp, sz, ctypes.POINTER(ci)]
            L.m2v_encode_resident420.argtypes = [vp, u32, u32, u32, vp, sz, ci, vp, sz, ctypes.POINTER(sz), vp]
            L.m2v_encode_resident420_begin.argtypes = [vp, u32, u32, u32, vp, sz, ci, vp, sz, vp]
            L.m2v_rgb_matrix.argtypes = [ci, ctypes.POINTER(ci), ctypes.POINTER(ci)]
            L.m2v_push_rgb.argtypes = [vp, u32, u32, u32, vp, sz, ci, ci]
            L.m2v_push_rgb_pull.restype = ctypes.c_longlong
            L.m2v_push_rgb_pull.argtypes = [vp, u32, u32, u32, vp, sz, ci, ci, vp, sz, ctypes.POINTER(ci)]
            L.m2v_encode_resident_rgb.argtypes = [vp, u32, u32, u32, vp, sz, ci, ci, vp, sz, ctypes.POINTER(sz), vp]
            L.m2v_encode_resident_rgb_begin.argtypes = [vp, u32, u32, u32, vp, sz, ci, ci, vp, sz, vp]
            L.m2v_set_frame_size.argtypes = [vp, ci, ci, ci]
            L.m2v_fit_size.argtypes = [ci, ci, ctypes.POINTER(u32), ctypes.POINTER(u32)]
            L.m2v_picture_stats.restype = ctypes.c_longlong
            L.m2v_picture_stats.argtypes = [vp, vp, sz]
            L.m2v_set_gop_levels.argtypes = [vp, vp, sz]
            L.m2v_gop_report.restype = ctypes.c_longlong
            L.m2v_gop_report.argtypes = [vp, vp, sz]
            L.m2v_set_gop_starts.argtypes = [vp, vp, sz]
            L.m2v_gop_layout.restype = ctypes.c_longlong
            L.m2v_gop_layout.argtypes = [u32, vp, sz, sz, vp]
            L.m2v_scene_report.restype = ctypes.c_longlong
            L.m2v_scene_report.argtypes = [vp, vp, sz]
            L.m2v_set_recon_out.argtypes = [vp, vp, sz, ci]
            L.m2v_stream_desc_module.restype = None
            L.m2v_stream_desc_module.argtypes = [ctypes.POINTER(StreamDesc)]
            L.m2v_set_stream_desc.argtypes = [vp, ctypes.POINTER(StreamDesc)]
            L.m2v_frame_rate_code.argtypes = [u32, u32]
            L.m2v_time_code.argtypes = [u32, u32, ctypes.POINTER(ctypes.c_uint8)]
            L.m2v_set_sequences.argtypes = [vp, vp, sz]
            L.m2v_sequence_report.argtypes = [vp, vp, sz]
            L.m2v_mux_bound.restype = sz
            L.m2v_mux_bound.argtypes = [ci, sz, sz]
            L.m2v_set_mux_out.argtypes = [vp, ci, vp, sz]
            L.m2v_mux_report.argtypes = [vp, vp, sz]
            L.m2v_mux_device.argtypes = [vp, ci, vp, vp, vp, sz, vp, sz, vp]
            L.m2v_mux_scan_tile.argtypes = []
            L.m2v_set_source_size.argtypes = [vp, ci, ci, ci]
            L.m2v_demux_bound.restype = sz
            L.m2v_demux_bound.argtypes = [vp, sz]
            L.m2v_demux_device.argtypes = [vp, ci, vp, vp, vp, sz, ci, vp, sz, vp, sz, vp]
            L.m2v_demux_report.argtypes = [vp, vp, sz]
            L.m2v_demux_scan_tile.argtypes = []
            L.m2v_decode_device.argtypes = [vp, vp, sz, vp, sz, ci, ci, vp]
            L.m2v_decode_report.argtypes = [vp, vp]
            L.m2v_decode_join_report.argtypes = [vp, vp]
            L.m2v_decode_conceal_report.argtypes = [vp, vp]
            L.m2v_decode_scan_tile.argtypes = []
            L.m2v_decode_streams_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, ci, ci, vp]
            L.m2v_decode_streams_report.argtypes = [vp, vp, sz]
            L.m2v_scale_taps.argtypes = [ci, ci, ci, ci, ctypes.POINTER(ci), ctypes.POINTER(ctypes.c_uint16)]
            L.m2v_decode_streams_main_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, ci, ctypes.c_uint, vp]
            L.m2v_decode_streams_main_ex_device.argtypes = [vp, vp, vp, vp, sz, vp, sz, ci, ctypes.c_uint, vp]
            L.m2v_deinterlace_device.argtypes = [vp, vp, sz, ci, ci, ci, ci, ci, ci, vp, sz, vp]
            L.m2v_deinterlace_bound.restype = ctypes.c_ulonglong
            L.m2v_deinterlace_bound.argtypes = [ci, ci, sz, ci]
            L.m2v_deinterlace_tile.argtypes = [ctypes.POINTER(ci), ctypes.POINTER(ci)]
        except AttributeError:
            # an OLDER build handed in through M2V_LIB for a same-box A/B (tools/ab.sh) may lack the newer entry points; the library of
            # this tree must have every one of them (tests/test_abi.py)
            if not os.environ.get("M2V_LIB"):
                raise
        _libs[path] = L
    return _libs[path]


def build(force=False, verbose=False):
    return _build.build(force=force, verbose=verbose)


def device_pci_bus_id(device=0):
    """PCI address of HIP device `device` as sysfs spells it ("0000:c1:00.0"), or None (m2v_device_pci_bus_id)"""
    buf = ctypes.create_string_buffer(64)
    n = lib().m2v_device_pci_bus_id(int(device), buf, 64)
    return buf.value.decode() if n > 0 else None


def _layout420(layout):
    """a name of LAYOUTS_420 or an M2V_420_* code -> the code (unknown codes pass through: the library answers M2V_E_PARAM)"""
    return LAYOUTS_420[layout] if isinstance(layout, str) else int(layout)


def to444(frames420, W, H, layout="i420"):
    """4:2:0 frames (uint8, W*H*3/2 bytes each) -> planar 4:4:4 [n, 3, H, W] with every chroma sample repeated 2 x 2: the frames
    whose stream a 4:2:0 encode equals by definition (include/m2v_mi355x.h).  numpy, host side: a reference, not a fast path."""
    code = _layout420(layout)
    f = np.ascontiguousarray(frames420, np.uint8).reshape(-1, W * H * 3 // 2)
    n, c = f.shape[0], W * H // 4
    if code < 2:
        a, b = f[:, W * H:W * H + c], f[:, W * H + c:]
    else:
        uv = f[:, W * H:].reshape(n, c, 2)
        a, b = uv[:, :, 0], uv[:, :, 1]
    u, v = (a, b) if code in (0, 2) else (b, a)
    out = np.empty((n, 3, H, W), np.uint8)
    out[:, 0] = f[:, :W * H].reshape(n, H, W)
    for k, p in ((1, u), (2, v)):
        out[:, k] = p.reshape(n, H // 2, W // 2).repeat(2, axis=1).repeat(2, axis=2)
    return out


def to420(frames444, layout="i420"):
    """planar 4:4:4 [n, 3, H, W] -> 4:2:0 frames [n, W*H*3/2] by the module's own down-conversion: mean2 = (a + b + 1) >> 1 over
    horizontal pairs, then over vertical pairs (RTL:1086-1089, 1167-1170).  to420(to444(x, l), l) == x."""
    code = _layout420(layout)
    f = np.asarray(frames444, np.uint8)
    n, _, H, W = f.shape
    c = f[:, 1:].astype(np.uint16)
    h = (c[..., 0::2] + c[..., 1::2] + 1) >> 1
    d = ((h[..., 0::2, :] + h[..., 1::2, :] + 1) >> 1).astype(np.uint8).reshape(n, 2, -1)
    a, b = (d[:, 0], d[:, 1]) if code in (0, 2) else (d[:, 1], d[:, 0])
    chroma = np.concatenate([a, b], axis=1) if code < 2 else np.stack([a, b], axis=2).reshape(n, -1)
    return np.concatenate([f[:, 0].reshape(n, -1), chroma], axis=1)


def _layout_rgb(layout):
    """a name of LAYOUTS_RGB or an M2V_RGB_* layout code -> the code (unknown codes pass through: the library answers M2V_E_PARAM)"""
    return LAYOUTS_RGB[layout] if isinstance(layout, str) else int(layout)


def _matrix_rgb(matrix):
    """a name of MATRICES_RGB or an M2V_RGB_* matrix code -> the code"""
    return MATRICES_RGB[matrix][0] if isinstance(matrix, str) else int(matrix)


def rgb_bytes_per_pixel(layout):
    return _RGB_FORM[_layout_rgb(layout)][0]


def rgb_to444(frames, W, H, layout="rgb24", matrix="bt601"):
    """RGB frames (uint8, W*H*bpp bytes each, one of LAYOUTS_RGB) -> planar 4:4:4 [n, 3, H, W] by the integer transform of
    include/m2v_mi355x.h: the frames whose stream an RGB encode equals by definition.  numpy integer arithmetic, host side: a
    reference, not a fast path."""
    code = _layout_rgb(layout)
    bpp, (o_r, o_g, o_b) = _RGB_FORM[code]
    _, T, yo = next(m for m in MATRICES_RGB.values() if m[0] == _matrix_rgb(matrix))
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, W * H * bpp)
    n = f.shape[0]
    if code == 6:
        px = f.reshape(n, 3, H * W)
        r, g, b = (px[:, k].astype(np.int32) for k in (o_r, o_g, o_b))
    else:
        px = f.reshape(n, H * W, bpp)
        r, g, b = (px[:, :, k].astype(np.int32) for k in (o_r, o_g, o_b))
    out = np.empty((n, 3, H, W), np.uint8)
    for k, off in enumerate((yo, 128, 128)):
        v = ((T[3 * k] * r + T[3 * k + 1] * g + T[3 * k + 2] * b + 8192) >> 14) + off          # (>> of a numpy int32 is arithmetic)
        out[:, k] = np.clip(v, 0, 255).astype(np.uint8).reshape(n, H, W)
    return out


# ---- frames of any size (m2v_set_frame_size, include/m2v_mi355x.h) ----
HEADER_MODES = {"module": 0, "true": 1}          # M2V_HEADER_*


def fit_size(w, h):
    """(xsize16, ysize16) of the whole macroblocks a w x h frame is padded to: ceil(/16) (m2v_fit_size)"""
    if w < 1 or h < 1:
        raise ValueError("fit_size: %d x %d" % (w, h))
    return (w + 15) // 16, (h + 15) // 16


def _planes(w, h, kind):
    """the planes of a w x h frame of `kind` ("444", a name of LAYOUTS_420 or of LAYOUTS_RGB), in memory order:
    [(element bytes, columns, rows, chroma?)]"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if kind in ("444", "rgbp"):
        return [(1, w, h, False)] * 3
    if kind in ("i420", "yv12"):
        return [(1, w, h, False), (1, cw, ch, True), (1, cw, ch, True)]
    if kind in ("nv12", "nv21"):
        return [(1, w, h, False), (2, cw, ch, True)]
    if kind in LAYOUTS_RGB:
        return [(_RGB_FORM[LAYOUTS_RGB[kind]][0], w, h, False)]
    raise ValueError("unknown kind of frame %r" % (kind,))


def frame_bytes(w, h, kind):
    """bytes of one w x h source frame of `kind`: "444", a name of LAYOUTS_420 or a name of LAYOUTS_RGB"""
    return sum(es * c * r for es, c, r, _ in _planes(w, h, kind))


def pad_frames(frames, w, h, kind):
    """w x h frames of `kind` -> [n, bytes] frames of the same kind at whole macroblocks, every plane extended to the right and then
    downwards by its last column and its last row: the frames whose stream an encode with a frame size set equals by definition
    (include/m2v_mi355x.h).  numpy, host side: a reference, not a fast path."""
    xs, ys = fit_size(w, h)
    W, H = 16 * xs, 16 * ys
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, frame_bytes(w, h, kind))
    n, out, at = f.shape[0], [], 0
    for es, c, r, chroma in _planes(w, h, kind):
        C, R = (W // 2, H // 2) if chroma else (W, H)
        p = f[:, at:at + es * c * r].reshape(n, r, c, es)
        at += es * c * r
        out.append(np.pad(p, ((0, 0), (0, R - r), (0, C - c), (0, 0)), mode="edge").reshape(n, -1))
    return np.ascontiguousarray(np.concatenate(out, axis=1))


# ---- frames of another size, resampled (m2v_set_source_size, include/m2v_mi355x.h) ----
SCALE_FILTERS = {"triangle": 0, "area": 1}       # M2V_SCALE_*
SCALE_MAXTAPS = 16                               # M2V_SCALE_MAXTAPS
SCALE_MAX_SIZE, SCALE_MAX_RATIO = 16384, 8


def _scale_filter(filter):
    code = SCALE_FILTERS.get(filter, filter)
    if code not in SCALE_FILTERS.values() or isinstance(code, bool):
        raise ValueError("unknown filter %r" % (filter,))
    return code


def scale_taps(filter, src, dst, x):
    """(first, [c(first), c(first + 1), ...]): the taps of output sample x of dst samples made from src samples, as the header defines
    them - weights a(i) > 0 of the triangle or the area, c(i) = floor(a(i) * 2^14 / sum a), the remainder onto the largest a(i) (the
    lowest i among equals).  Python integers, written from the definition: m2v_scale_taps is held against it."""
    code = _scale_filter(filter)
    if not (1 <= src <= SCALE_MAX_SIZE and 1 <= dst <= SCALE_MAX_SIZE and 0 <= x < dst) or src > SCALE_MAX_RATIO * dst:
        raise ValueError("scale_taps: %d -> %d, sample %d" % (src, dst, x))
    if code == 0:
        P, R = (2 * x + 1) * src - dst, 2 * max(src, dst)
        a = [(i, R - abs(2 * dst * i - P)) for i in range((P - R) // (2 * dst), (P + R) // (2 * dst) + 2)]
    else:
        a = [(i, min((i + 1) * dst, (x + 1) * src) - max(i * dst, x * src)) for i in range(x * src // dst, (x + 1) * src // dst + 1)]
    a = [(i, v) for i, v in a if v > 0]
    assert a and all(j[0] == i[0] + 1 for i, j in zip(a, a[1:]))
    A = sum(v for _, v in a)
    c = [v * (1 << 14) // A for _, v in a]
    c[max(range(len(a)), key=lambda k: (a[k][1], -k))] += (1 << 14) - sum(c)
    return a[0][0], c


@functools.lru_cache(maxsize=64)
def _scale_table(code, src, dst):
    """the taps of every output sample as arrays [dst, n]: the samples they read (clamped to the plane) and their coefficients (0
    beyond a sample's own count)"""
    taps = [scale_taps(code, src, dst, x) for x in range(dst)]
    n = max(len(c) for _, c in taps)
    idx, coef = np.zeros((dst, n), np.int64), np.zeros((dst, n), np.int64)
    for x, (first, c) in enumerate(taps):
        idx[x] = np.clip(first + np.arange(n), 0, src - 1)
        coef[x, :len(c)] = c
    return idx, coef


def scale_frames(frames, sw, sh, w, h, kind, filter="triangle"):
    """sw x sh frames of `kind` -> [n, bytes] frames of the same kind at w x h, every plane resampled on its own (4:2:0 chroma in the
    4:2:0 domain), every byte of an element with its plane's taps: the horizontal pass on every source row,
    t = (sum c * s + 128) >> 8, then the vertical pass, o = (sum d * t + 2^19) >> 20.  The frames whose padded form (pad_frames) an
    encode with a source size set codes, by definition (include/m2v_mi355x.h).  numpy, host side: a reference, not a fast path."""
    code = _scale_filter(filter)
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, frame_bytes(sw, sh, kind))
    n, out, at = f.shape[0], [], 0
    for (es, c, r, _), (_, C, R, _) in zip(_planes(sw, sh, kind), _planes(w, h, kind)):
        p = f[:, at:at + es * c * r].reshape(n, r, c, es).astype(np.int64)
        at += es * c * r
        ix, cx = _scale_table(code, c, C)
        iy, cy = _scale_table(code, r, R)
        t = sum(p[:, :, ix[:, k], :] * cx[None, None, :, k, None] for k in range(ix.shape[1]))
        t = (t + 128) >> 8
        o = sum(t[:, iy[:, k], :, :] * cy[None, :, k, None, None] for k in range(iy.shape[1]))
        o = (o + (1 << 19)) >> 20
        assert o.min() >= 0 and o.max() <= 255
        out.append(o.astype(np.uint8).reshape(n, -1))
    return np.ascontiguousarray(np.concatenate(out, axis=1))


# ---- woven frames to progressive frames (m2v_deinterlace_device, include/m2v_mi355x.h) ----
DEINT_MODES = {"line": 0, "adaptive": 1, "blend": 2}      # M2V_DEINT_LINE / ADAPTIVE / BLEND
DEINT_RATES = {"frame": 0, "field": 1}                    # M2V_DEINT_FRAME_RATE / FIELD_RATE
DEINT_ORDERS = {"tff": 0, "bff": 1}                       # M2V_DEINT_TFF / BFF
DEINT_MAX_SIZE = 16384


def _deint_code(table, what, value):
    code = table.get(value, value) if isinstance(value, str) else value
    if isinstance(code, bool) or code not in table.values():
        raise ValueError("unknown %s %r" % (what, value))
    return int(code)


def deinterlace_bound(w, h, nframes, rate="frame"):
    """m2v_deinterlace_bound: the bytes a deinterlace_device of nframes w x h frames writes; 0 for illegal arguments"""
    return int(lib().m2v_deinterlace_bound(int(w), int(h), int(nframes), DEINT_RATES.get(rate, rate) if isinstance(rate, str) else int(rate)))


def deinterlace_tile():
    """m2v_deinterlace_tile: (bytes of a row, rows) after which the device deinterlacer hands over to another group of lanes"""
    c, r = ctypes.c_int(0), ctypes.c_int(0)
    lib().m2v_deinterlace_tile(ctypes.byref(c), ctypes.byref(r))
    return int(c.value), int(r.value)


def deinterlace_frames(frames, w, h, layout="i420", mode="adaptive", rate="frame", order="tff"):
    """woven w x h 4:2:0 frames of `layout` -> [n or 2 n, bytes] progressive frames of the same size and layout, as the header defines
    them: every plane alone and bytewise, row r of any plane in the field of parity r & 1; the fields of the call one sequence in time,
    F[k] in frame k >> 1 with parity order ^ (k & 1), an absent field replaced by the nearest of its parity; the rows of the output
    field's parity kept, the others sp = (c + e + 1) >> 1 of the kept rows beside them ("line"), sp clamped to d +- m around the mean
    of the neighbouring fields by the motion found ("adaptive"), or every row (up + 2 s + down + 2) >> 2 ("blend", frame rate only).
    The frames a deinterlace_device returns, by definition (include/m2v_mi355x.h).  numpy, host side: a reference, not a fast path."""
    m, fr, o = _deint_code(DEINT_MODES, "mode", mode), _deint_code(DEINT_RATES, "rate", rate), _deint_code(DEINT_ORDERS, "order", order)
    name = layout if isinstance(layout, str) else {v: k for k, v in LAYOUTS_420.items()}.get(int(layout))
    if name not in LAYOUTS_420:
        raise ValueError("unknown layout %r" % (layout,))
    if m == 2 and fr == 1:
        raise ValueError("deinterlace_frames: \"blend\" knows no fields, so it has no field rate")
    if not (1 <= w <= DEINT_MAX_SIZE and 2 <= h <= DEINT_MAX_SIZE):
        raise ValueError("deinterlace_frames: %d x %d" % (w, h))
    f = np.ascontiguousarray(frames, np.uint8).reshape(-1, frame_bytes(w, h, name))
    n, nf = f.shape[0], 2 * f.shape[0]
    if not n:
        return f.copy()
    ks = range(0, nf, 1 if fr else 2)
    out, at = [], 0

    def sub(k):             # a field index outside the call: the nearest field of the same parity inside it
        return k & 1 if k < 0 else nf - 2 + (k & 1) if k >= nf else k
    for es, c, r, _ in _planes(w, h, name):
        s = f[:, at:at + es * c * r].reshape(n, r, es * c).astype(np.int64)
        at += es * c * r
        if r < 2:
            o_ = s[[k >> 1 for k in ks]]
        elif m == 2:
            o_ = (s[:, np.maximum(np.arange(r) - 1, 0)] + 2 * s + s[:, np.minimum(np.arange(r) + 1, r - 1)] + 2) >> 2
        else:
            rows = np.arange(r)
            yc = np.where(rows - 1 >= 0, rows - 1, rows + 1)
            ye = np.where(rows + 1 < r, rows + 1, rows - 1)
            o_ = np.empty((len(ks), r, es * c), np.int64)
            for j, k in enumerate(ks):
                p = o ^ (k & 1)
                cur = s[k >> 1]
                C, E = cur[yc], cur[ye]
                sp = (C + E + 1) >> 1
                if m == 1:
                    b, a = s[sub(k - 1) >> 1], s[sub(k + 1) >> 1]
                    pp, nn = s[sub(k - 2) >> 1], s[sub(k + 2) >> 1]
                    d = (b + a) >> 1
                    t0 = np.abs(b - a) >> 1
                    t1 = (np.abs(pp[yc] - C) + np.abs(pp[ye] - E)) >> 1
                    t2 = (np.abs(nn[yc] - C) + np.abs(nn[ye] - E)) >> 1
                    mm = np.maximum(t0, np.maximum(t1, t2))
                    sp = np.minimum(np.maximum(sp, d - mm), d + mm)
                o_[j] = np.where(((rows & 1) == p)[:, None], cur, sp)
        assert o_.min() >= 0 and o_.max() <= 255
        out.append(o_.astype(np.uint8).reshape(len(ks), -1))
    return np.ascontiguousarray(np.concatenate(out, axis=1))


def planes_of_recon(buf, w, h, layout="i420"):
    """Frames of m2v_set_recon_out (`buf`: a numpy array or torch tensor of n * frame_bytes(w, h, layout) bytes, w x h the size set or the
    coded size) -> (Y [n, h, w], U, V [n, (h + 1) / 2, (w + 1) / 2]): views where the layout allows it (the interleaved ones are strided)."""
    name = layout if isinstance(layout, str) else {v: k for k, v in LAYOUTS_420.items()}[int(layout)]
    if name not in LAYOUTS_420:
        raise ValueError("planes_of_recon: unknown layout %r" % (layout,))
    cw, ch = (w + 1) // 2, (h + 1) // 2
    f = buf.reshape(-1, frame_bytes(w, h, name))
    n = f.shape[0]
    y = f[:, :w * h].reshape(n, h, w)
    if name in ("i420", "yv12"):
        a, b = f[:, w * h:w * h + cw * ch].reshape(n, ch, cw), f[:, w * h + cw * ch:].reshape(n, ch, cw)
    else:
        uv = f[:, w * h:].reshape(n, ch, cw, 2)
        a, b = uv[..., 0], uv[..., 1]
    return (y, a, b) if name in ("i420", "nv12") else (y, b, a)


def set_header_size(stream, w, h):
    """a copy of an encoder stream (bytes) with the four size fields rewritten: horizontal / vertical size of sequence_header (12 + 12
    bits, bytes 4 - 6) and display size of sequence_display_extension (14 + 1 + 14 bits from byte 30).  What M2V_HEADER_TRUE writes."""
    if not (0 < w < 4096 and 0 < h < 4096):
        raise ValueError("set_header_size: %d x %d" % (w, h))
    b = bytearray(stream)
    assert bytes(b[0:4]) == b"\x00\x00\x01\xb3" and bytes(b[22:26]) == b"\x00\x00\x01\xb5" and b[26] >> 4 == 2, "not a stream of this encoder"
    b[4:7] = ((w << 12) | h).to_bytes(3, "big")
    keep = b[33] & 7
    b[30:34] = ((((w << 15) | (1 << 14) | h) << 3) | keep).to_bytes(4, "big")
    return bytes(b)


def clamp_geometry(xsize16, ysize16, XL=7, YL=7):
    """Clamped (W, H) of RTL/mpeg2encoder.v:985-1006 (pure host arithmetic)."""
    def c(s, L):
        s &= (2 << L) - 1
        lim = 1 << L
        return lim - 1 if s > lim else 3 if s < 4 else s - 1
    return 16 * (c(xsize16, XL) + 1), 16 * (c(ysize16, YL) + 1)


class Mpeg2Encoder:
    """`mpeg2encoder #(XL, YL, VECTOR_LEVEL, Q_LEVEL)` on one MI355X (RTL/mpeg2encoder.v:10-38)."""

    def __init__(self, XL=6, YL=6, VECTOR_LEVEL=3, Q_LEVEL=2, device=0, debug=False):
        self.params = (XL, YL, VECTOR_LEVEL, Q_LEVEL)
        self.device = device
        self._geom = {}
        # what is set on the handle, as the setters below take it back (_for_call): the three options, the lists, the buffers, the size
        self._set = {"stats": False, "gop_bytes_max": 0, "scene_cut": 0, "gop_levels": None, "gop_starts": None, "sequences": None,
                     "stream_desc": None, "recon_out": None, "mux_out": None, "frame_size": None, "source_size": None}
        err = ctypes.c_int(0)
        self._L = lib(debug)
        self._h = self._L.m2v_create(XL, YL, VECTOR_LEVEL, Q_LEVEL, device, ctypes.byref(err))
        if not self._h:
            raise M2VError("m2v_create failed with code %d (parameters %r, device %d): %s"
                           % (err.value, self.params, device, self._L.m2v_last_error(None).decode()))

    def close(self):
        if getattr(self, "_h", None):
            self._L.m2v_destroy(self._h)
            self._h = None

    __del__ = close

    def _chk(self, r, what):
        if r < 0:
            raise M2VError("%s failed (%d): %s" % (what, r, self._L.m2v_last_error(self._h).decode()))
        return r

    def reset(self):
        """m2v_reset (`rstn` low, RTL:1028-1039): whatever is in flight on the handle is waited for and dropped, the handle is idle again"""
        self._chk(self._L.m2v_reset(self._h), "m2v_reset")

    def set_option(self, name, value):
        self._chk(self._L.m2v_set_option(self._h, name.encode(), int(value)), "m2v_set_option(%s)" % name)
        if name == "stats":
            self._set[name] = bool(value)
        if name in ("gop_bytes_max", "scene_cut", "decode_syntax", "decode_b_pictures", "decode_interlaced", "decode_extended", "decode_mb_tools", "decode_field_pictures", "decode_join", "decode_conceal"):
            self._set[name] = int(value)

    def _set_list(self, key, values, ctype, what):
        """a setter that takes a list of unsigned integers; None or an empty list clears it"""
        name = "m2v_set_" + key
        v, buf = _uint_list(values, ctype, M2VError("%s failed (-1): %s" % (name, what)))
        self._chk(getattr(self._L, name)(self._h, buf, len(v)), name)
        self._set[key] = v or None

    def _pop(self, fn, dtype, max_records):
        """the waiting records of one report function, oldest first, at most max_records of them, as a numpy structured array"""
        report = getattr(self._L, fn)
        n = self._chk(report(self._h, None, 0), fn)
        if max_records is not None:
            n = min(n, int(max_records))
        out = np.zeros(n, dtype)
        if n:
            n = self._chk(report(self._h, out.ctypes.data, n), fn)
        return out[:n]

    @contextlib.contextmanager
    def _for_call(self, settings):
        """`settings` (keys of self._set, values as the setters take them) for the duration of a call: the handle's own are back afterwards"""
        def apply(key, v):
            if key in ("stats", "gop_bytes_max", "scene_cut"):
                self.set_option(key, v)
            elif key == "frame_size":
                self.set_frame_size(*(v or (0, 0, 0)))
            elif key == "source_size":
                self.set_source_size(*(v or (0, 0, 0)))
            elif key == "recon_out":
                self.set_recon_out(*(v or (None, 0)))
            elif key == "mux_out":
                self.set_mux_out(*(v or (None,)))
            else:
                getattr(self, "set_" + key)(v)
        before = {key: self._set[key] for key in settings}
        try:
            for key, v in settings.items():
                apply(key, v)
            yield
        finally:
            for key, v in before.items():
                apply(key, v)

    def set_gop_starts(self, frames):
        """m2v_set_gop_starts: in every sequence started from now on a GOP also starts at each of these frame numbers (strictly
        ascending; M2VError otherwise, and the previous setting stays); None or an empty sequence clears the setting.  Not the
        module's behaviour."""
        self._set_list("gop_starts", frames, ctypes.c_uint32, "a frame number is 0 .. 2^32 - 1")

    def scene_report(self, max_records=None):
        """Pops the waiting records of m2v_scene_report, oldest first, at most max_records of them: a numpy structured array of
        SCENE_STAT_DTYPE - one per picture of a sequence that had a list of GOP starts or option "scene_cut", empty otherwise."""
        return self._pop("m2v_scene_report", SCENE_STAT_DTYPE, max_records)

    def set_sequences(self, lengths):
        """m2v_set_sequences: the frames of every resident call started from now on are len(lengths) clips of these many frames, each
        coded as a stream of its own (sequence_report says where); None or an empty sequence clears the setting.  A call whose frames
        are not the sum of the entries, or an entry of 0, fails with M2VError when it starts."""
        self._set_list("sequences", lengths, ctypes.c_uint32, "an entry is 1 .. 2^32 - 1 frames")

    def sequence_report(self, max_records=None):
        """Pops the waiting records of m2v_sequence_report, oldest first, at most max_records of them: a numpy structured array of
        SEQUENCE_STAT_DTYPE - one per clip of the last resident call that had a list of two or more entries, empty otherwise."""
        return self._pop("m2v_sequence_report", SEQUENCE_STAT_DTYPE, max_records)

    def set_gop_levels(self, levels):
        """m2v_set_gop_levels: GOP k of every sequence started from now on is coded at levels[min(k, len - 1)], each 1..4 (M2VError
        otherwise, and the previous setting stays); None or an empty sequence clears the setting.  Not the module's behaviour."""
        self._set_list("gop_levels", levels, ctypes.c_uint8, "a level is 1..4")

    def gop_report(self, max_records=None):
        """Pops the waiting records of option "gop_bytes_max" (m2v_gop_report), oldest first, at most max_records of them: a numpy
        structured array of GOP_STAT_DTYPE, empty while the cap is off."""
        return self._pop("m2v_gop_report", GOP_STAT_DTYPE, max_records)

    def set_recon_out(self, ptr, cap, layout="i420"):
        """m2v_set_recon_out: every resident sequence started from now on writes its reconstructed pictures, frame n at
        ptr + n * frame_bytes(w, h, layout), into the `cap` bytes of device memory at `ptr`; ptr = None or 0 clears the setting.  Idle
        handles only.  planes_of_recon takes the buffer apart."""
        self._chk(self._L.m2v_set_recon_out(self._h, ptr or None, int(cap), _layout420(layout)), "m2v_set_recon_out")
        self._set["recon_out"] = (int(ptr), int(cap), layout) if ptr else None

    def set_mux_out(self, kind, ptr=None, cap=0):
        """m2v_set_mux_out: every resident call started from now on also leaves its stream as a transport ("ts") or program ("ps")
        stream in the `cap` bytes of device memory at `ptr` - one container per clip of a batch, each on a 32-byte boundary;
        mux_report says where.  kind = None or 0 clears the setting.  Idle handles only."""
        k = _mux_kind(kind) if kind else 0
        self._chk(self._L.m2v_set_mux_out(self._h, k, (ptr or None) if k else None, int(cap) if k else 0), "m2v_set_mux_out")
        self._set["mux_out"] = (k, int(ptr), int(cap)) if k else None

    def mux_report(self, max_records=None):
        """Pops the waiting records of m2v_mux_report, oldest first, at most max_records of them: a numpy structured array of
        MUX_STAT_DTYPE - one per container of the last resident call that had a container buffer set, or of the last mux_device."""
        return self._pop("m2v_mux_report", MUX_STAT_DTYPE, max_records)

    def mux_device(self, es, kind, segments=None, out=None, cap=None, pictures=None):
        """m2v_mux_device: the elementary streams in the uint8 device tensor `es` - the whole tensor, or the (offset, bytes) pairs of
        `segments`, at any byte alignment - as transport ("ts") or program ("ps") streams, muxed on the device.  Returns
        (out, records): the containers in the one-dimensional uint8 tensor `out` on es's device (allocated from m2v_mux_bound when not
        given; `pictures` = an upper bound of the pictures of all streams together, counted on the device when not given), of which at
        most `cap` bytes are written (default: all of it), and their records (mux_report): container b is
        out[out_offset : out_offset + out_bytes] where status is MUX_OK."""
        import torch
        if not isinstance(es, torch.Tensor) or es.dtype != torch.uint8 or es.dim() != 1 or not es.is_cuda or es.device.index != self.device:
            raise ValueError("mux_device: a one-dimensional uint8 tensor on the handle's device is required")
        if es.stride(0) != 1:
            raise ValueError("mux_device: the tensor must be contiguous")
        k = _mux_kind(kind)
        seg = [(0, es.numel())] if segments is None else [(int(a), int(b)) for a, b in segments]
        if not seg or any(a < 0 or b < 0 or a + b > es.numel() for a, b in seg):
            raise ValueError("mux_device: a segment lies outside the tensor, or there is none")
        if out is None:
            if pictures is None and es.numel() >= 4:       # picture_start_codes anywhere in the tensor: an upper bound of the pictures
                pictures = int(((es[:-3] == 0) & (es[1:-2] == 0) & (es[2:-1] == 1) & (es[3:] == 0)).sum().item())
            total = sum(b for _, b in seg)
            out = torch.empty(mux_bound(k, total, pictures or 1) + (32 + 1024) * len(seg), dtype=torch.uint8, device=es.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != es.device or out.dim() != 1 or out.stride(0) != 1:
            raise ValueError("mux_device: out must be a contiguous one-dimensional uint8 tensor on the stream's device")
        cap = out.numel() if cap is None else int(cap)
        if cap < 0 or cap > out.numel():
            raise ValueError("mux_device: cap is 0 .. out.numel()")
        off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
        nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
        self._chk(self._L.m2v_mux_device(self._h, k, es.data_ptr(), off, nb, len(seg), out.data_ptr(), cap,
                                         torch.cuda.current_stream(es.device).cuda_stream), "m2v_mux_device")
        return out, self.mux_report()

    def demux_report(self, max_records=None):
        """Pops the waiting records of m2v_demux_report, oldest first, at most max_records of them: a numpy structured array of
        DEMUX_STAT_DTYPE - one per container of the last demux_device."""
        return self._pop("m2v_demux_report", DEMUX_STAT_DTYPE, max_records)

    def demux_device(self, src, kind, segments=None, stream=None, out=None, stamps=False, cap=None, stamp_cap=None):
        """m2v_demux_device: the transport ("ts") or program ("ps") streams in the uint8 device tensor `src` - the whole tensor, or the
        (offset, bytes) pairs of `segments`, at any byte alignment - back to the video elementary stream of each, demultiplexed on the
        device: the inverse of mux_device.  stream: the PID / stream_id to take, None: found in each container.  Returns (out, records)
        or, with stamps, (out, records, stamps): the streams in the one-dimensional uint8 tensor `out` on src's device (allocated from
        m2v_demux_bound when not given), of which at most `cap` bytes are written (default: all of it), their records (demux_report):
        stream b is out[out_offset : out_offset + out_bytes] where status is DEMUX_OK, and one DEMUX_STAMP_DTYPE record per PES packet as
        an int64 device tensor [n, 4] (es_offset, pts, dts, src_offset; -1 = absent), the containers' stamps one behind the other;
        stamp_cap: room for that many (None: one per transport packet / per nine bytes of program stream, always enough)."""
        import torch
        if not isinstance(src, torch.Tensor) or src.dtype != torch.uint8 or src.dim() != 1 or not src.is_cuda or src.device.index != self.device:
            raise ValueError("demux_device: a one-dimensional uint8 tensor on the handle's device is required")
        if src.stride(0) != 1 and src.numel() > 1:
            raise ValueError("demux_device: the tensor must be contiguous")
        k = _mux_kind(kind)
        seg = [(0, src.numel())] if segments is None else [(int(a), int(b)) for a, b in segments]
        if not seg or any(a < 0 or b < 0 or a + b > src.numel() for a, b in seg):
            raise ValueError("demux_device: a segment lies outside the tensor, or there is none")
        if out is None:
            out = torch.empty(max(demux_bound([b for _, b in seg]), 32), dtype=torch.uint8, device=src.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != src.device or out.dim() != 1 or out.stride(0) != 1:
            raise ValueError("demux_device: out must be a contiguous one-dimensional uint8 tensor on the containers' device")
        cap = out.numel() if cap is None else int(cap)
        if cap < 0 or cap > out.numel():
            raise ValueError("demux_device: cap is 0 .. out.numel()")
        st = None
        if stamps:
            if stamp_cap is None:       # a PES packet starts in a transport packet of its own / takes at least nine bytes of a program stream
                stamp_cap = sum(b // 188 + 1 if k == MUX_KINDS["ts"] else b // 9 + 1 for _, b in seg)
            st = torch.empty((max(int(stamp_cap), 1), 4), dtype=torch.int64, device=src.device)
        off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
        nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
        self._chk(self._L.m2v_demux_device(self._h, k, src.data_ptr() or None, off, nb, len(seg), -1 if stream is None else int(stream),
                                           out.data_ptr(), cap, st.data_ptr() if st is not None else None, int(stamp_cap) if st is not None else 0,
                                           torch.cuda.current_stream(src.device).cuda_stream), "m2v_demux_device")
        r = self.demux_report()
        if st is None:
            return out, r
        return out, r, st[:min(int(stamp_cap), int(r["pes_packets"].sum()))]

    def decode_report(self):
        """m2v_decode_report: the record of the last decode_device on this handle, a numpy record of DECODE_STAT_DTYPE"""
        out = np.zeros(1, DECODE_STAT_DTYPE)
        self._chk(self._L.m2v_decode_report(self._h, out.ctypes.data), "m2v_decode_report")
        return out[0]

    def decode_join_report(self):
        """m2v_decode_join_report: the join record of the last decode_device on this handle, a numpy record of DECODE_JOIN_DTYPE - the
        join point, the offset the tail was cut at, the frames dropped in front and behind; 0, es_bytes, 0, 0 with option "decode_join"
        off and for a refused stream"""
        out = np.zeros(1, DECODE_JOIN_DTYPE)
        self._chk(self._L.m2v_decode_join_report(self._h, out.ctypes.data), "m2v_decode_join_report")
        return out[0]

    def decode_conceal_report(self):
        """m2v_decode_conceal_report: the concealment report of the last decode_device on this handle, a numpy record of
        DECODE_CONCEAL_DTYPE - the picture start code of the first damaged picture, the slices dropped, the rows concealed, those of
        them without a frame in front, the pictures with such a row; es_bytes, 0, 0, 0, 0 with option "decode_conceal" off and for a
        call that did not answer M2V_DEC_OK"""
        out = np.zeros(1, DECODE_CONCEAL_DTYPE)
        self._chk(self._L.m2v_decode_conceal_report(self._h, out.ctypes.data), "m2v_decode_conceal_report")
        return out[0]

    def decode_device(self, es, layout="i420", mode="iso", out=None, container=None, stream=None, syntax="module", b_pictures=False, interlaced=False, extended=False, mb_tools=False, field_pictures=False, join=0, conceal=False):
        """m2v_decode_device: the MPEG-2 elementary stream in the one-dimensional uint8 device tensor `es` (at any byte alignment) decoded
        on the device to 4:2:0 frames in `layout`; mode "iso" is decoder.decode(quirks=False), "module" the module's own loop
        (quirks=True).  Returns (frames [pictures, frame_bytes] uint8 on es's device, record).  out: a contiguous uint8 tensor to write into
        (all of it is the capacity); None: the call probes the stream first and allocates.  A status other than M2V_DEC_OK raises
        M2VError, whose text names the status and err_offset (decode_report still answers the record).

        container = "ts" or "ps": `es` is one transport or program stream; it is demultiplexed on the device (demux_device, `stream` as
        there) into a scratch tensor on the same HIP stream, and that is decoded.  The demux record is read once before the decode
        call: one host wait of 64 bytes, which the decode's own probe pays anyway.  A demux status other than DEMUX_OK raises M2VError
        naming the status and err_offset.  The scratch tensor is zeroed first and the stream handed on with the zero padding to a whole
        32-byte word that the encoder writes behind sequence_end_code and a muxer drops: the decoder's definition wants it.  Without
        the keyword the function is exactly what it was.

        syntax = "module" (the default) or "main": the call decodes with that syntax whatever set_option("decode_syntax") left on the
        handle - the option is set for this call and afterwards put back to the value it had.  "main": Main-Profile streams
        of progressive I / P frame pictures from any encoder (decoder.decode(..., quirks=False, syntax="main") is the definition; mode
        must be "iso").  It goes with container= as well: a transport stream from an ordinary multiplexer, demultiplexed and decoded
        on the device.

        b_pictures = True (with syntax="main"; ValueError otherwise): option "decode_b_pictures" for this call, put back afterwards as
        syntax= is - B pictures are decoded too and the frames come in display order
        (decoder.decode(..., quirks=False, syntax="main", b_pictures=True) is the definition).  False, the default, decodes without
        the option whatever set_option("decode_b_pictures") left on the handle.

        interlaced = True (with syntax="main", b_pictures either way; ValueError otherwise): option "decode_interlaced" for this call, put
        back afterwards as b_pictures= is - frame pictures with frame_pred_frame_dct 0 are decoded too: field prediction and field DCT,
        one frame per coded picture with both fields woven (decoder.decode(..., quirks=False, syntax="main", interlaced=True) is the
        definition).  False, the default, decodes without the option whatever set_option("decode_interlaced") left on the handle.

        extended = True (with syntax="main", the other two either way; ValueError otherwise): option "decode_extended" for this call, put
        back afterwards as interlaced= is - several slices in a macroblock row, slice headers with intra_slice_flag 1,
        quant_matrix_extension and composite_display_flag 1 are read too (decoder.decode(..., quirks=False, syntax="main",
        extended=True) is the definition).  False, the default, decodes without the option whatever set_option("decode_extended")
        left on the handle.

        mb_tools = True (with extended=True; ValueError otherwise): option "decode_mb_tools" for this call, put back afterwards as
        extended= is - Table B-15 for intra blocks (intra_vlc_format 1), concealment motion vectors and dual prime are read too
        (decoder.decode(..., quirks=False, syntax="main", extended=True, mb_tools=True) is the definition).  False, the default,
        decodes without the option whatever set_option("decode_mb_tools") left on the handle.

        field_pictures = True (with interlaced=True, extended=True and mb_tools=True, b_pictures either way; ValueError otherwise): option
        "decode_field_pictures" for this call, put back afterwards as mb_tools= is - pictures with picture_structure 1 / 2 are read too,
        two field pictures woven into one frame, the record counted in frames (decoder.decode(..., quirks=False, syntax="main",
        interlaced=True, extended=True, mb_tools=True, field_pictures=True) is the definition).  False, the default, decodes without the
        option whatever set_option("decode_field_pictures") left on the handle.

        join = 0 .. 3, "head" (1), "tail" (2) or "both" (3) (other than 0 with field_pictures=True and what it needs; ValueError
        otherwise): option "decode_join" for this call, put back afterwards as field_pictures= is - a stream cut from a running
        broadcast: "head" reads from the first sequence header on and drops the B pictures whose anchors are not there, "tail" leaves
        out the frame the stream breaks off in (decoder.decode(..., field_pictures=True, join=...) is the definition;
        decode_join_report answers what was left out).  With container= the stream is what the demultiplexer extracts, and the join
        record's offsets count in it.  0, the default, decodes without the option whatever set_option("decode_join") left on the
        handle.

        conceal = True (with field_pictures=True and what it needs, join 0 .. 3; ValueError otherwise): option "decode_conceal" for this
        call, put back afterwards as join= is - a damaged slice is dropped and its macroblock row patched from the frame in front
        instead of refusing the stream (decoder.decode(..., field_pictures=True, join=..., conceal=True) is the definition;
        decode_conceal_report answers what was patched).  False, the default, decodes without the option whatever
        set_option("decode_conceal") left on the handle."""
        import torch
        if conceal and not field_pictures:
            raise ValueError("decode_device: conceal goes with field_pictures=True")
        if isinstance(join, str):
            if join not in DEC_JOINS:
                raise ValueError("decode_device: join is 0 .. 3 or one of %s" % ", ".join(DEC_JOINS))
            join = DEC_JOINS[join]
        if join not in (0, 1, 2, 3):
            raise ValueError("decode_device: join is 0 .. 3 or one of %s" % ", ".join(DEC_JOINS))
        if join and not field_pictures:
            raise ValueError("decode_device: join goes with field_pictures=True")
        if syntax not in DEC_SYNTAXES:
            raise ValueError("decode_device: syntax is one of %s" % ", ".join(DEC_SYNTAXES))
        if b_pictures and syntax != "main":
            raise ValueError("decode_device: b_pictures goes with syntax=\"main\"")
        if interlaced and syntax != "main":
            raise ValueError("decode_device: interlaced goes with syntax=\"main\"")
        if extended and syntax != "main":
            raise ValueError("decode_device: extended goes with syntax=\"main\"")
        if mb_tools and not extended:
            raise ValueError("decode_device: mb_tools goes with extended=True")
        if field_pictures and not (interlaced and extended and mb_tools):
            raise ValueError("decode_device: field_pictures goes with interlaced=True, extended=True and mb_tools=True")
        held_c = self._set.get("decode_conceal", 0)                        # what set_option("decode_conceal") left on the handle
        if int(bool(conceal)) != held_c:
            self.set_option("decode_conceal", int(bool(conceal)))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced,
                                          extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_conceal", held_c)
        held_j = self._set.get("decode_join", 0)                           # what set_option("decode_join") left on the handle
        if int(join) != held_j:
            self.set_option("decode_join", int(join))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced,
                                          extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_join", held_j)
        held_f = self._set.get("decode_field_pictures", 0)                 # what set_option("decode_field_pictures") left on the handle
        if int(bool(field_pictures)) != held_f:
            self.set_option("decode_field_pictures", int(bool(field_pictures)))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced,
                                          extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_field_pictures", held_f)
        held_t = self._set.get("decode_mb_tools", 0)                       # what set_option("decode_mb_tools") left on the handle
        if int(bool(mb_tools)) != held_t:
            self.set_option("decode_mb_tools", int(bool(mb_tools)))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced,
                                          extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_mb_tools", held_t)
        held_x = self._set.get("decode_extended", 0)                       # what set_option("decode_extended") left on the handle
        if int(bool(extended)) != held_x:
            self.set_option("decode_extended", int(bool(extended)))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced,
                                          extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_extended", held_x)
        held_i = self._set.get("decode_interlaced", 0)                     # what set_option("decode_interlaced") left on the handle
        if int(bool(interlaced)) != held_i:
            self.set_option("decode_interlaced", int(bool(interlaced)))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced, extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_interlaced", held_i)
        held_b = self._set.get("decode_b_pictures", 0)                     # what set_option("decode_b_pictures") left on the handle
        if int(bool(b_pictures)) != held_b:
            self.set_option("decode_b_pictures", int(bool(b_pictures)))
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced, extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_b_pictures", held_b)
        held = self._set.get("decode_syntax", DEC_SYNTAXES["module"])      # what set_option("decode_syntax") left on the handle
        if DEC_SYNTAXES[syntax] != held:
            self.set_option("decode_syntax", DEC_SYNTAXES[syntax])
            try:
                return self.decode_device(es, layout=layout, mode=mode, out=out, container=container, stream=stream, syntax=syntax, b_pictures=b_pictures, interlaced=interlaced, extended=extended, mb_tools=mb_tools, field_pictures=field_pictures, join=join, conceal=conceal)
            finally:
                self.set_option("decode_syntax", held)
        if container is not None:
            if not isinstance(es, torch.Tensor) or es.dtype != torch.uint8 or es.dim() != 1 or not es.is_cuda or es.device.index != self.device:
                raise ValueError("decode_device: a one-dimensional uint8 tensor on the handle's device is required")
            if es.stride(0) != 1 and es.numel() > 1:
                raise ValueError("decode_device: the tensor must be contiguous")
            scratch = torch.zeros(demux_bound([es.numel()]) + 32, dtype=torch.uint8, device=es.device)
            _, r = self.demux_device(es, container, stream=stream, out=scratch)
            if r["status"][0] != DEMUX_OK:
                raise M2VError("m2v_demux_device: %s (%d), err_offset %d" % (DEMUX_STATUS.get(int(r["status"][0]), "?"), r["status"][0],
                                                                            r["err_offset"][0]))
            es = scratch[int(r["out_offset"][0]):int(r["out_offset"][0]) + (int(r["out_bytes"][0]) + 31) // 32 * 32]
        elif stream is not None:
            raise ValueError("decode_device: stream needs a container")
        if not isinstance(es, torch.Tensor) or es.dtype != torch.uint8 or es.dim() != 1 or not es.is_cuda or es.device.index != self.device:
            raise ValueError("decode_device: a one-dimensional uint8 tensor on the handle's device is required")
        if es.stride(0) != 1 and es.numel() > 1:
            raise ValueError("decode_device: the tensor must be contiguous")
        code = _layout420(layout)
        m = DEC_MODES[mode] if isinstance(mode, str) else int(mode)
        stream = torch.cuda.current_stream(es.device).cuda_stream

        def call(ptr, cap):
            self._chk(self._L.m2v_decode_device(self._h, es.data_ptr(), es.numel(), ptr, cap, code, m, stream), "m2v_decode_device")
            r = self.decode_report()
            if r["status"] != DEC_OK:
                raise M2VError("m2v_decode_device: %s (%d), err_offset %d" % (DEC_STATUS.get(int(r["status"]), "?"), r["status"], r["err_offset"]))
            return r
        if out is None:
            r = call(None, 0)
            out = torch.empty(int(r["pictures"]) * int(r["frame_bytes"]), dtype=torch.uint8, device=es.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != es.device or not out.is_contiguous():
            raise ValueError("decode_device: out must be a contiguous uint8 tensor on the stream's device")
        r = call(out.data_ptr() or None, out.numel()) if out.numel() else call(None, 0)
        n, fb = int(r["pictures"]), int(r["frame_bytes"])
        return out.reshape(-1)[:n * fb].reshape(n, fb), r

    def deinterlace_device(self, frames, width, height, layout="i420", mode="adaptive", rate="frame", order="tff", out=None, stream=None):
        """m2v_deinterlace_device: the woven width x height 4:2:0 frames in the uint8 device tensor `frames` (whole frames of `layout` back
        to back, as decode_device returns them; any byte alignment) deinterlaced on the device: mode "line", "adaptive" or "blend", rate
        "frame" (a frame per frame) or "field" (a frame per field, in time order), order "tff" or "bff" (the parity of the field that is
        first in time, for the whole call).  deinterlace_frames is the definition.  Returns the frames [n or 2 n, frame_bytes] as a uint8
        tensor on the same device: `out` (a contiguous uint8 tensor, all of it the capacity) or a new one.  One launch, ordered on `stream` (a
        torch stream; None: the current one) like any torch operation, no host wait."""
        import torch
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or not frames.is_cuda or frames.device.index != self.device:
            raise ValueError("deinterlace_device: a uint8 tensor on the handle's device is required")
        if not frames.is_contiguous():
            raise ValueError("deinterlace_device: the tensor must be contiguous")
        m, fr, o = _deint_code(DEINT_MODES, "mode", mode), _deint_code(DEINT_RATES, "rate", rate), _deint_code(DEINT_ORDERS, "order", order)
        code = _layout420(layout)
        width, height = int(width), int(height)
        fb = width * height + 2 * ((width + 1) // 2) * ((height + 1) // 2)
        if width < 1 or height < 2 or frames.numel() % fb:
            raise ValueError("deinterlace_device: %d bytes are no whole frames of %d x %d" % (frames.numel(), width, height))
        n = frames.numel() // fb
        nout = n * (2 if fr else 1)
        if out is None:
            out = torch.empty(nout * fb, dtype=torch.uint8, device=frames.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != frames.device or not out.is_contiguous():
            raise ValueError("deinterlace_device: out must be a contiguous uint8 tensor on the frames' device")
        s = torch.cuda.current_stream(frames.device) if stream is None else stream
        run_on = s
        if not s.cuda_stream:
            # the null stream has no handle the entry could take (NULL there means the handle's own stream, which the null stream does not
            # wait for): the launch goes to a stream of this object's that waits for the null stream, and the null stream then waits for it
            if getattr(self, "_deint_stream", None) is None:
                self._deint_stream = torch.cuda.Stream(frames.device)
            run_on = self._deint_stream
            run_on.wait_stream(s)
        try:
            self._chk(self._L.m2v_deinterlace_device(self._h, frames.data_ptr() or None, n, width, height, code, m, fr, o, out.data_ptr() or None,
                                                     out.numel(), run_on.cuda_stream), "m2v_deinterlace_device")
        finally:
            if run_on is not s:
                s.wait_stream(run_on)
        return out.reshape(-1)[:nout * fb].reshape(nout, fb)

    def decode_streams_report(self, max_records=None):
        """Pops the waiting records of m2v_decode_streams_report, oldest first, at most max_records of them: a numpy structured array
        of DECODE_STREAM_STAT_DTYPE - one per stream of the last decode_streams."""
        return self._pop("m2v_decode_streams_report", DECODE_STREAM_STAT_DTYPE, max_records)

    def decode_streams(self, es, segments, layout="i420", mode="iso", out=None, container=None, stream=None, syntax="module", b_pictures=False,
                       interlaced=False, extended=False, mb_tools=False):
        """m2v_decode_streams_device: the elementary streams at the (offset, bytes) pairs of `segments` in the one-dimensional uint8
        device tensor `es` - at any byte alignment, of any picture sizes - decoded on the device in one call.  Returns (frames, records):
        a one-dimensional uint8 tensor on es's device and a structured array of DECODE_STREAM_STAT_DTYPE, one record per stream;
        frames_of_stream(frames, records[b]) is stream b's [pictures, frame_bytes] view.  A stream that is refused does NOT raise: its
        record says so (rec.status, rec.err_offset relative to the stream), and the others are decoded.  out: a contiguous uint8
        tensor to write into (all of it is the capacity; a stream whose room does not lie inside it is DEC_OVERFLOW); None: the call
        probes the streams first and allocates.  ValueError for bad arguments.

        container = "ts" or "ps": `es` and `segments` are containers; they go through demux_device (`stream` as there) in one call into
        a zeroed scratch tensor, and every stream is handed on with the zero padding to a whole 32-byte word, as decode_device(container=)
        does.  A container the demultiplexer refused comes back as DEC_SYNTAX with pictures 0.

        syntax = "main": m2v_decode_streams_main_device - the streams are main-syntax streams (what an ordinary multiplexer's
        containers hold), each judged as decode_device(syntax="main", b_pictures=, interlaced=) judges it alone; with b_pictures the
        frames of a stream are in display order.  The syntax is the call's: the handle's three decode options are neither read nor
        changed.  The mode is "iso" there ("module" is a ValueError), and b_pictures / interlaced need syntax="main".

        extended / mb_tools: m2v_decode_streams_main_ex_device - each stream judged as decode_device(syntax="main", ..., extended=,
        mb_tools=) judges it alone: several slices a row, slice header extras, quant_matrix_extension, composite_display_flag 1; on
        top of those Table B-15, concealment vectors and dual prime.  extended needs syntax="main" and mb_tools needs extended
        (ValueError); with both False the call is the one it was."""
        import torch
        if syntax not in ("module", "main"):
            raise ValueError("decode_streams: syntax is \"module\" or \"main\"")
        if syntax != "main" and (b_pictures or interlaced):
            raise ValueError("decode_streams: b_pictures and interlaced need syntax=\"main\"")
        if extended and syntax != "main":
            raise ValueError("decode_streams: extended needs syntax=\"main\"")
        if mb_tools and not extended:
            raise ValueError("decode_streams: mb_tools needs extended")
        if syntax == "main" and mode in ("module", DEC_MODES["module"]):
            raise ValueError("decode_streams: with syntax=\"main\" the mode is \"iso\"")
        if not isinstance(es, torch.Tensor) or es.dtype != torch.uint8 or es.dim() != 1 or not es.is_cuda or es.device.index != self.device:
            raise ValueError("decode_streams: a one-dimensional uint8 tensor on the handle's device is required")
        if es.stride(0) != 1 and es.numel() > 1:
            raise ValueError("decode_streams: the tensor must be contiguous")
        try:
            seg = [(int(a), int(b)) for a, b in segments]
        except (TypeError, ValueError):
            raise ValueError("decode_streams: segments are (offset, bytes) pairs")
        if not 1 <= len(seg) <= 65535 or any(a < 0 or b < 0 or a + b > es.numel() for a, b in seg):
            raise ValueError("decode_streams: 1 .. 65535 segments inside the tensor are required")
        if container is not None:
            scratch = torch.zeros(demux_bound([b for _, b in seg]) + 32, dtype=torch.uint8, device=es.device)
            _, r = self.demux_device(es, container, segments=seg, stream=stream, out=scratch)
            es = scratch
            seg = [(int(q["out_offset"]), (int(q["out_bytes"]) + 31) // 32 * 32) if q["status"] == DEMUX_OK else (0, 0) for q in r]
        elif stream is not None:
            raise ValueError("decode_streams: stream needs a container")
        if mode not in DEC_MODES and not isinstance(mode, int):
            raise ValueError("decode_streams: mode is one of %s" % ", ".join(DEC_MODES))
        if layout not in LAYOUTS_420 and not isinstance(layout, int):
            raise ValueError("decode_streams: layout is one of %s" % ", ".join(LAYOUTS_420))
        code = _layout420(layout)
        m = DEC_MODES[mode] if isinstance(mode, str) else int(mode)
        off = (ctypes.c_uint64 * len(seg))(*[a for a, _ in seg])
        nb = (ctypes.c_uint64 * len(seg))(*[b for _, b in seg])
        hip_stream = torch.cuda.current_stream(es.device).cuda_stream

        flags = (DECS_B_PICTURES if b_pictures else 0) | (DECS_INTERLACED if interlaced else 0)

        def call(ptr, cap):
            if extended:
                x = flags | DECS_EXTENDED | (DECS_MB_TOOLS if mb_tools else 0)
                self._chk(self._L.m2v_decode_streams_main_ex_device(self._h, es.data_ptr() or None, off, nb, len(seg), ptr, cap, code, x, hip_stream),
                          "m2v_decode_streams_main_ex_device")
            elif syntax == "main":
                self._chk(self._L.m2v_decode_streams_main_device(self._h, es.data_ptr() or None, off, nb, len(seg), ptr, cap, code, flags, hip_stream),
                          "m2v_decode_streams_main_device")
            else:
                self._chk(self._L.m2v_decode_streams_device(self._h, es.data_ptr() or None, off, nb, len(seg), ptr, cap, code, m, hip_stream),
                          "m2v_decode_streams_device")
            return self.decode_streams_report()
        if out is None:
            r = call(None, 0)
            out = torch.empty(int((r["out_offset"] + r["rec"]["out_bytes"]).max()), dtype=torch.uint8, device=es.device)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != es.device or not out.is_contiguous():
            raise ValueError("decode_streams: out must be a contiguous uint8 tensor on the streams' device")
        r = call(out.data_ptr() or None, out.numel()) if out.numel() else call(None, 0)
        return out.reshape(-1), r

    def set_stream_desc(self, desc):
        """m2v_set_stream_desc: what every sequence started from now on says about itself in its sequence headers and time codes - a
        StreamDesc (stream_desc builds one); None sets the module's values again.  Idle handles only; M2VError for a value out of
        range, and the previous setting stays.  Not the module's behaviour."""
        if desc is not None and not isinstance(desc, StreamDesc):
            raise M2VError("m2v_set_stream_desc failed (-1): a StreamDesc or None is required")
        self._chk(self._L.m2v_set_stream_desc(self._h, ctypes.byref(desc) if desc is not None else None), "m2v_set_stream_desc")
        self._set["stream_desc"] = StreamDesc.from_buffer_copy(desc) if desc is not None else None

    def set_frame_size(self, w, h, header="module"):
        """m2v_set_frame_size: from now on every whole-frame entry takes w x h frames in its own format and pads them on the device;
        header "module" (the padded size in the stream's headers) or "true" (w x h).  (0, 0) switches it off.  Idle handles only."""
        code = HEADER_MODES[header] if isinstance(header, str) else int(header)
        self._chk(self._L.m2v_set_frame_size(self._h, int(w), int(h), code), "m2v_set_frame_size")
        self._set["frame_size"] = (int(w), int(h), code) if w or h else None

    @property
    def frame_size(self):
        """(w, h, header code) set by set_frame_size, or None"""
        return self._set["frame_size"]

    def set_source_size(self, sw, sh, filter="triangle"):
        """m2v_set_source_size: from now on every resident whole-frame entry takes sw x sh frames in its own format and resamples them
        on the device to the picture size - the size of set_frame_size, or of the call's xsize16, ysize16 - with filter "triangle" or
        "area" (scale_frames says what comes out).  (0, 0) switches it off.  Idle handles only."""
        code = SCALE_FILTERS[filter] if isinstance(filter, str) else int(filter)
        self._chk(self._L.m2v_set_source_size(self._h, int(sw), int(sh), code), "m2v_set_source_size")
        self._set["source_size"] = (int(sw), int(sh), code) if sw or sh else None

    @property
    def source_size(self):
        """(sw, sh, filter code) set by set_source_size, or None"""
        return self._set["source_size"]

    def _fb(self, xsize16, ysize16, kind):
        """bytes of one frame a whole-frame entry takes: of the size set, else of the clamped geometry"""
        w, h = self.frame_size[:2] if self.frame_size else self.geometry(xsize16, ysize16)
        return frame_bytes(w, h, kind)

    def geometry(self, xsize16, ysize16):
        # (a handle's clamps are fixed at creation: asked once per size - the per-call bindings below are on a caller's critical path)
        got = self._geom.get((xsize16, ysize16))
        if got is None:
            w, h = ctypes.c_int(), ctypes.c_int()
            self._chk(self._L.m2v_geometry(self._h, xsize16, ysize16, ctypes.byref(w), ctypes.byref(h)), "m2v_geometry")
            got = self._geom[(xsize16, ysize16)] = (w.value, h.value)
        return got

    @staticmethod
    def _flat_u8(a):
        """the array as contiguous bytes: itself when it already is (no copy, no new object beyond a view)"""
        if isinstance(a, np.ndarray) and a.dtype == np.uint8 and a.flags["C_CONTIGUOUS"]:
            return a
        return np.ascontiguousarray(a, np.uint8)

    # ---- port-level interface ----
    def push_beats(self, xsize16, ysize16, pframes_count, y4, u4, v4, stop_with_last=False):
        y4 = np.ascontiguousarray(y4, np.uint8).reshape(-1)
        u4 = np.ascontiguousarray(u4, np.uint8).reshape(-1)
        v4 = np.ascontiguousarray(v4, np.uint8).reshape(-1)
        assert y4.size == u4.size == v4.size and y4.size % 4 == 0
        self._chk(self._L.m2v_push_beats(self._h, xsize16, ysize16, pframes_count, y4.ctypes.data, u4.ctypes.data,
                                         v4.ctypes.data, y4.size // 4, int(bool(stop_with_last))), "m2v_push_beats")

    PACKED = {"yuv24": (0, 3), "uyv24": (1, 3), "yuvx32": (2, 4), "ayuv32": (3, 4)}

    def push_packed(self, xsize16, ysize16, pframes_count, pixels, layout="yuv24", stop_with_last=False):
        """pixels: packed 4:4:4 samples in raster order ([..., bytes_per_pixel] uint8), a multiple of 4 pixels."""
        code, bpp = self.PACKED[layout]
        p = np.ascontiguousarray(pixels, np.uint8).reshape(-1)
        assert p.size % (4 * bpp) == 0
        self._chk(self._L.m2v_push_packed(self._h, xsize16, ysize16, pframes_count, p.ctypes.data, p.size // (4 * bpp),
                                          code, int(bool(stop_with_last))), "m2v_push_packed")

    def push_frames(self, xsize16, ysize16, pframes_count, frames444):
        fb = self._fb(xsize16, ysize16, "444")
        f = self._flat_u8(frames444)
        assert f.size % fb == 0
        self._chk(self._L.m2v_push_frames(self._h, xsize16, ysize16, pframes_count, f.ctypes.data,
                                          f.size // fb), "m2v_push_frames")

    def push_frames_pull(self, xsize16, ysize16, pframes_count, frames444, dst, offset=0):
        """m2v_push_frames_pull: push_frames + pull_into(dst, offset) in one call, the stream bytes copied while the frames upload:
        -> (bytes written, last)"""
        fb = self._fb(xsize16, ysize16, "444")
        f = self._flat_u8(frames444)
        assert f.size % fb == 0
        assert dst.dtype == np.uint8 and dst.flags["C_CONTIGUOUS"]
        last = ctypes.c_int(0)
        n = self._chk(self._L.m2v_push_frames_pull(self._h, xsize16, ysize16, pframes_count, f.ctypes.data, f.size // fb,
                                                   dst.ctypes.data + offset, (dst.size - offset) & ~31, ctypes.byref(last)), "m2v_push_frames_pull")
        return n, bool(last.value)

    def push_frames420(self, xsize16, ysize16, pframes_count, frames420, layout="i420"):
        """m2v_push_frames420: whole 4:2:0 frames (W*H*3/2 bytes each) in one of LAYOUTS_420"""
        fb = self._fb(xsize16, ysize16, "i420")
        f = self._flat_u8(frames420)
        assert f.size % fb == 0
        self._chk(self._L.m2v_push_frames420(self._h, xsize16, ysize16, pframes_count, f.ctypes.data, f.size // fb,
                                             _layout420(layout)), "m2v_push_frames420")

    def push_frames420_pull(self, xsize16, ysize16, pframes_count, frames420, dst, offset=0, layout="i420"):
        """m2v_push_frames420_pull: push_frames420 + pull_into(dst, offset) in one call -> (bytes written, last)"""
        fb = self._fb(xsize16, ysize16, "i420")
        f = self._flat_u8(frames420)
        assert f.size % fb == 0
        assert dst.dtype == np.uint8 and dst.flags["C_CONTIGUOUS"]
        last = ctypes.c_int(0)
        n = self._chk(self._L.m2v_push_frames420_pull(self._h, xsize16, ysize16, pframes_count, f.ctypes.data, f.size // fb,
                                                      _layout420(layout), dst.ctypes.data + offset, (dst.size - offset) & ~31,
                                                      ctypes.byref(last)), "m2v_push_frames420_pull")
        return n, bool(last.value)

    def push_rgb(self, xsize16, ysize16, pframes_count, frames, layout="rgb24", matrix="bt601"):
        """m2v_push_rgb: whole RGB frames (W*H*3 or W*H*4 bytes each) in one of LAYOUTS_RGB, converted with one of MATRICES_RGB"""
        f = self._flat_u8(frames)
        fb = self._fb(xsize16, ysize16, "rgb24" if rgb_bytes_per_pixel(layout) == 3 else "rgbx")
        assert f.size % fb == 0
        self._chk(self._L.m2v_push_rgb(self._h, xsize16, ysize16, pframes_count, f.ctypes.data, f.size // fb, _layout_rgb(layout),
                                       _matrix_rgb(matrix)), "m2v_push_rgb")

    def push_rgb_pull(self, xsize16, ysize16, pframes_count, frames, dst, offset=0, layout="rgb24", matrix="bt601"):
        """m2v_push_rgb_pull: push_rgb + pull_into(dst, offset) in one call -> (bytes written, last)"""
        f = self._flat_u8(frames)
        fb = self._fb(xsize16, ysize16, "rgb24" if rgb_bytes_per_pixel(layout) == 3 else "rgbx")
        assert f.size % fb == 0
        assert dst.dtype == np.uint8 and dst.flags["C_CONTIGUOUS"]
        last = ctypes.c_int(0)
        n = self._chk(self._L.m2v_push_rgb_pull(self._h, xsize16, ysize16, pframes_count, f.ctypes.data, f.size // fb, _layout_rgb(layout),
                                                _matrix_rgb(matrix), dst.ctypes.data + offset, (dst.size - offset) & ~31,
                                                ctypes.byref(last)), "m2v_push_rgb_pull")
        return n, bool(last.value)

    def upload_wait(self):
        """option direct_upload = 2: returns when every frame handed to push_frames so far has been read"""
        self._chk(self._L.m2v_upload_wait(self._h), "m2v_upload_wait")

    def sequence_stop(self):
        self._chk(self._L.m2v_sequence_stop(self._h), "m2v_sequence_stop")

    @property
    def busy(self):
        return bool(self._L.m2v_busy(self._h))

    def pull(self, max_bytes=1 << 20):
        """-> (bytes, last)"""
        # one buffer per handle, kept: a fresh 16 MB numpy array per call is a fresh mapping whose pages fault in one by one
        buf = getattr(self, "_pullbuf", None)
        if buf is None or buf.size < (max_bytes & ~31):
            buf = self._pullbuf = np.empty(max_bytes & ~31, np.uint8)
        last = ctypes.c_int(0)
        n = self._chk(self._L.m2v_pull(self._h, buf.ctypes.data, max_bytes & ~31, ctypes.byref(last)), "m2v_pull")
        return buf[:n].tobytes(), bool(last.value)

    def pull_into(self, dst, offset=0):
        """m2v_pull straight into the caller's uint8 array (from `offset` on, whole 32-byte words): -> (bytes written, last).  What a
        C caller does: no intermediate object."""
        assert dst.dtype == np.uint8 and dst.flags["C_CONTIGUOUS"]
        last = ctypes.c_int(0)
        n = self._chk(self._L.m2v_pull(self._h, dst.ctypes.data + offset, (dst.size - offset) & ~31, ctypes.byref(last)), "m2v_pull")
        return n, bool(last.value)

    def pull_all(self):
        out = []
        while True:
            b, last = self.pull()
            out.append(b)
            if last or not b:
                break
        return b"".join(out)

    def encode(self, frames444, xsize16, ysize16, pframes_count, nbeats=None, layout=None, matrix="bt601"):
        """One whole sequence from host memory through the beat interface; returns the stream bytes.
        layout (a name of LAYOUTS_420 or LAYOUTS_RGB): `frames444` holds whole 4:2:0 or RGB frames instead; matrix (a name of
        MATRICES_RGB) converts the latter."""
        W, H = self.geometry(xsize16, ysize16)
        if layout is not None:
            assert nbeats is None, "there are no 4:2:0 or RGB beats"
            if layout in LAYOUTS_RGB:
                self.push_rgb(xsize16, ysize16, pframes_count, frames444, layout, matrix)
            else:
                self.push_frames420(xsize16, ysize16, pframes_count, frames444, layout)
            self.sequence_stop()
            return self.pull_all()
        if self.frame_size:
            assert nbeats is None, "there are no partial frames while a frame size is set"
            self.push_frames(xsize16, ysize16, pframes_count, frames444)
            self.sequence_stop()
            return self.pull_all()
        f = np.ascontiguousarray(frames444, np.uint8).reshape(-1, 3, H * W)
        bpf = W * H // 4
        total = f.shape[0] * bpf if nbeats is None else nbeats
        full = total // bpf
        if full:
            self.push_frames(xsize16, ysize16, pframes_count, f[:full])
        rem = total - full * bpf
        if rem:
            fr = f[full]
            self.push_beats(xsize16, ysize16, pframes_count, fr[0][:rem * 4], fr[1][:rem * 4], fr[2][:rem * 4])
        self.sequence_stop()
        return self.pull_all()

    # ---- HBM-resident interface (what bench.py times) ----
    def encode_resident(self, d_frames_ptr, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, stream=0):
        n = ctypes.c_size_t(0)
        self._chk(self._L.m2v_encode_resident(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes,
                                              d_out_ptr, cap, ctypes.byref(n), stream), "m2v_encode_resident")
        return n.value

    def encode_resident_begin(self, d_frames_ptr, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, stream=0):
        """enqueue a whole sequence and return; encode_resident_end() waits for it and returns the byte count"""
        self._chk(self._L.m2v_encode_resident_begin(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes, d_out_ptr, cap,
                                                    stream), "m2v_encode_resident_begin")

    def encode_resident420(self, d_frames_ptr, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, layout="i420", stream=0):
        """m2v_encode_resident420: `nframes` 4:2:0 frames at a 16-byte aligned device pointer"""
        n = ctypes.c_size_t(0)
        self._chk(self._L.m2v_encode_resident420(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes, _layout420(layout),
                                                 d_out_ptr, cap, ctypes.byref(n), stream), "m2v_encode_resident420")
        return n.value

    def encode_resident420_begin(self, d_frames_ptr, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, layout="i420", stream=0):
        """enqueue a whole 4:2:0 sequence and return; encode_resident_end() waits for it and returns the byte count"""
        self._chk(self._L.m2v_encode_resident420_begin(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes,
                                                       _layout420(layout), d_out_ptr, cap, stream), "m2v_encode_resident420_begin")

    def encode_resident_rgb(self, d_frames_ptr, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, layout="rgb24", matrix="bt601",
                            stream=0):
        """m2v_encode_resident_rgb: `nframes` RGB frames at a 16-byte aligned device pointer"""
        n = ctypes.c_size_t(0)
        self._chk(self._L.m2v_encode_resident_rgb(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes, _layout_rgb(layout),
                                                  _matrix_rgb(matrix), d_out_ptr, cap, ctypes.byref(n), stream), "m2v_encode_resident_rgb")
        return n.value

    def encode_resident_rgb_begin(self, d_frames_ptr, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, layout="rgb24",
                                  matrix="bt601", stream=0):
        """enqueue a whole RGB sequence and return; encode_resident_end() waits for it and returns the byte count"""
        self._chk(self._L.m2v_encode_resident_rgb_begin(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes,
                                                        _layout_rgb(layout), _matrix_rgb(matrix), d_out_ptr, cap, stream),
                  "m2v_encode_resident_rgb_begin")

    def picture_stats(self, max_records=None):
        """Pops the waiting records of option "stats" (m2v_picture_stats), oldest first, at most max_records of them: a numpy structured
        array of PICTURE_STAT_DTYPE, empty while the option is off."""
        return self._pop("m2v_picture_stats", PICTURE_STAT_DTYPE, max_records)

    def encode_tensor(self, frames, pframes_count, order="rgb", matrix="bt601", out=None, header=None, stats=False, gop_levels=None,
                      gop_bytes_max=0, gop_starts=None, scene_cut=0, recon=None, desc=None, sequences=None, container=None, size=None,
                      filter="triangle"):
        """One whole sequence from a torch image tensor on the handle's device, in one call: contiguous uint8 [N, H, W, 3] (order
        "rgb" / "bgr"), [N, H, W, 4] ("rgbx" / "bgrx" / "xrgb" / "xbgr") or [N, 3, H, W] ("rgb": planar).  Runs
        m2v_encode_resident_rgb on torch's current stream and returns the stream bytes as a uint8 device tensor (a view of `out` when
        given; M2VError when it is too small).  ValueError for any other tensor.
        header = "true" or "module": H, W of any size the handle can pad to (set_frame_size for the duration of the call; the handle's
        own setting is back afterwards), and what the stream's headers say of a size that is not whole macroblocks - "true": the
        tensor's size, what a player is to show; "module": the padded size, the module's stream for the padded frames.  Without the
        keyword H and W must be whole macroblocks, as ever: padding is asked for, never a surprise for a caller that relied on the
        ValueError.
        stats=True: returns (stream, records) - the sequence's picture records (picture_stats; option "stats" for the duration of the
        call, the handle's own setting is back afterwards).
        gop_levels = a sequence of levels 1..4, gop_bytes_max = B > 0: a level per GOP and a byte cap per GOP for this call
        (set_gop_levels, option "gop_bytes_max"; the handle's own settings are back afterwards).  The cap's records wait for
        gop_report().
        gop_starts = a strictly ascending sequence of frame numbers, scene_cut = T > 0: where GOPs start in this call besides the cadence
        (set_gop_starts, option "scene_cut"; the handle's own settings are back afterwards).  The records wait for scene_report().
        recon = "i420", "yv12", "nv12" or "nv21": the reconstructed pictures too, as a uint8 tensor [N, frame_bytes(W, H, recon)] on the
        frames' device, returned after the stream (and after the records with stats=True); planes_of_recon takes it apart
        (set_recon_out for the duration of the call; the handle's own setting is back afterwards).
        desc = a StreamDesc (stream_desc): what the stream says about itself, for this call (set_stream_desc; the handle's own setting
        is back afterwards).  The matrix does not set it: matrix="bt709" goes with desc=stream_desc(colour="bt709").
        sequences = a list of frame counts that add up to N (ValueError otherwise): the frames are that many clips, each coded as a
        stream of its own, one behind the other on 32-byte boundaries in the tensor returned (set_sequences for the duration of the
        call; the handle's own setting is back afterwards).  sequence_report() says where each one is; encode_batch does both.
        container = "ts" or "ps": the first element returned is the transport or program stream, muxed on the device, instead of the
        elementary stream (set_mux_out for the duration of the call; the handle's own setting is back afterwards): the bytes of
        container.mux_ts / mux_ps of the elementary stream.  With sequences the tensor holds one container per clip and mux_report()
        says where each one is; encode_batch does both.  M2VError if the muxer refuses the stream.
        size = (w, h): the picture size; the tensor's own H, W are then a source size and its frames are resampled to w x h on the
        device with filter = "triangle" or "area" (set_source_size for the duration of the call; the handle's own settings are back
        afterwards).  header, recon and the stream's geometry go by w x h: a picture size that is not whole macroblocks still needs
        header=.  Without the keyword the tensor is the picture, whatever source size the handle holds."""
        import torch
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() != 4:
            raise ValueError("encode_tensor: a uint8 tensor of 4 dimensions is required")
        if not frames.is_cuda or frames.device.index != self.device:
            raise ValueError("encode_tensor: the tensor is on %s, the handle on device %d" % (frames.device, self.device))
        if not frames.is_contiguous():
            raise ValueError("encode_tensor: the tensor must be contiguous")
        if matrix not in MATRICES_RGB:
            raise ValueError("encode_tensor: unknown matrix %r" % (matrix,))
        N, d1, d2, d3 = frames.shape
        if sequences is not None:
            sequences = check_sequences(sequences, N)
        if order in ("rgb", "bgr") and d3 == 3:
            layout, H, W = order + "24", d1, d2
        elif order in ("rgbx", "bgrx", "xrgb", "xbgr") and d3 == 4:
            layout, H, W = order, d1, d2
        elif order == "rgb" and d1 == 3:
            layout, H, W = "rgbp", d2, d3
        else:
            raise ValueError("encode_tensor: shape %r does not go with order %r" % (tuple(frames.shape), order))
        if header is not None and header not in HEADER_MODES:
            raise ValueError("encode_tensor: unknown header %r" % (header,))
        if recon is not None and recon not in LAYOUTS_420:
            raise ValueError("encode_tensor: unknown recon layout %r" % (recon,))
        if filter not in SCALE_FILTERS:
            raise ValueError("encode_tensor: unknown filter %r" % (filter,))
        source = None
        if size is not None:
            try:
                pw, ph = (int(v) for v in size)
            except (TypeError, ValueError):
                raise ValueError("encode_tensor: size is (w, h), not %r" % (size,)) from None
            if not (1 <= W <= SCALE_MAX_SIZE and 1 <= H <= SCALE_MAX_SIZE) or pw < 1 or ph < 1 or W > SCALE_MAX_RATIO * pw or H > SCALE_MAX_RATIO * ph:
                raise ValueError("encode_tensor: %d x %d frames do not resample to %d x %d (1 ... %d either way, at most %d times the picture)"
                                 % (W, H, pw, ph, SCALE_MAX_SIZE, SCALE_MAX_RATIO))
            source, W, H = (W, H, filter), pw, ph
        xs, ys = (W + 15) // 16, (H + 15) // 16
        if header is None and (H % 16 or W % 16):
            raise ValueError("encode_tensor: %d x %d is not whole macroblocks; header=\"true\" or \"module\" pads it on the device" % (W, H))
        if W < 1 or H < 1 or self.geometry(xs, ys) != (16 * xs, 16 * ys):
            raise ValueError("encode_tensor: %d x %d does not pad to a size of this handle (64 ... %d x 64 ... %d)"
                             % (W, H, 16 << self.params[0], 16 << self.params[1]))
        if out is None:
            out = torch.empty(N * (3 * 256 * xs * ys + 34) + (1 << 16) + 64 * len(sequences or ()), dtype=torch.uint8, device=frames.device)     # (34: repeat_headers)
        elif not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.device != frames.device or not out.is_contiguous() or out.dim() != 1:
            raise ValueError("encode_tensor: out must be a contiguous one-dimensional uint8 tensor on the frames' device")
        rec = torch.empty((N, frame_bytes(W, H, recon)), dtype=torch.uint8, device=frames.device) if recon is not None else None
        mux = None
        if container is not None:
            nclips = len(sequences or ()) or 1
            mux = torch.empty(mux_bound(container, out.numel(), N) + 32 * nclips, dtype=torch.uint8, device=frames.device)
        # what the call sets, in the cases it always has: a tensor of whole macroblocks clears a size the handle holds
        fit = bool(W % 16 or H % 16)
        call = {}
        if fit or self.frame_size:
            call["frame_size"] = (W, H, header) if fit else None
        if source or self.source_size:
            call["source_size"] = source
        if stats and not self._set["stats"]:
            call["stats"] = 1
        if sequences is not None:
            call["sequences"] = sequences
        if desc is not None:
            call["stream_desc"] = desc
        if gop_levels is not None:
            call["gop_levels"] = gop_levels
        if gop_bytes_max:
            call["gop_bytes_max"] = gop_bytes_max
        if gop_starts is not None:
            call["gop_starts"] = gop_starts
        if scene_cut:
            call["scene_cut"] = scene_cut
        if rec is not None:
            call["recon_out"] = (rec.data_ptr(), rec.numel(), recon)
        if mux is not None:
            call["mux_out"] = (container, mux.data_ptr(), mux.numel())
        with self._for_call(call):
            nb = self.encode_resident_rgb(frames.data_ptr(), N, out.data_ptr(), out.numel(), xs, ys, pframes_count, layout, matrix,
                                          stream=torch.cuda.current_stream(frames.device).cuda_stream)
            records = self.picture_stats() if stats else None
        first = out[:nb]
        if mux is not None:
            r = self.mux_report()
            if len(r) == 0 or (r["status"] != MUX_OK).any():
                raise M2VError("encode_tensor: the muxer refused the stream (status %r)" % (r["status"].tolist(),))
            if sequences is None or len(sequences) < 2:
                first = mux[:int(r["out_bytes"][0])]
            else:
                self._mux_records = r
                first = mux[:int(r["out_offset"][-1] + r["out_bytes"][-1])]
        res = (first,) + ((records,) if stats else ()) + ((rec,) if rec is not None else ())
        return res if len(res) > 1 else res[0]

    def encode_batch(self, frames, pframes_count, lengths=None, **kw):
        """A batch of clips in one call, one stream per clip: a uint8 tensor [B, N, H, W, C] (or [B, N, 3, H, W]) on the handle's
        device - B clips of N frames - or a 4-D tensor of frames as encode_tensor takes it with lengths = the clips' frame counts.
        Returns (stream_tensor, offsets): clip b's stream is stream_tensor[offsets[b]:offsets[b + 1]], offsets a list of B + 1 ints,
        every one a multiple of 32.  Keywords as encode_tensor's; with stats or recon the first element of its tuple is the stream.
        With container = "ts" or "ps" the tensor holds the clips' containers instead and the second element is a list of
        (offset, bytes) per clip: clip b's container is stream_tensor[offset:offset + bytes], every offset a multiple of 32."""
        import torch
        if not isinstance(frames, torch.Tensor) or frames.dim() not in (4, 5):
            raise ValueError("encode_batch: a uint8 tensor of 4 or 5 dimensions is required")
        if frames.dim() == 5:
            if lengths is not None:
                raise ValueError("encode_batch: lengths go with a 4-D tensor; a 5-D one says them itself")
            if not frames.is_contiguous():
                raise ValueError("encode_batch: the tensor must be contiguous")
            lengths = [frames.shape[1]] * frames.shape[0]
            frames = frames.reshape((frames.shape[0] * frames.shape[1],) + tuple(frames.shape[2:]))
        elif lengths is None:
            raise ValueError("encode_batch: a 4-D tensor needs lengths")
        lengths = check_sequences(lengths, frames.shape[0])
        res = self.encode_tensor(frames, pframes_count, sequences=lengths, **kw)
        stream = res[0] if isinstance(res, tuple) else res
        if kw.get("container") is not None:
            offsets = [(0, int(stream.numel()))] if len(lengths) < 2 else [(int(o), int(b)) for o, b in zip(self._mux_records["out_offset"],
                                                                                                          self._mux_records["out_bytes"])]
        elif len(lengths) < 2:           # (a list of one entry is no batch: one stream, from 0 to its end)
            offsets = [0, int(stream.numel())]
        else:
            rec = self.sequence_report()
            offsets = [int(v) for v in rec["offset"]] + [int(rec["offset"][-1] + rec["bytes"][-1])]
        return ((stream, offsets) + tuple(res[1:])) if isinstance(res, tuple) else (stream, offsets)

    def encode_resident_end(self):
        n = ctypes.c_size_t(0)
        self._chk(self._L.m2v_encode_resident_end(self._h, ctypes.byref(n)), "m2v_encode_resident_end")
        return n.value

    # ---- strip mode (config c5): see include/m2v_mi355x.h ----
    def strip_begin(self, d_frames_ptr, nframes, xsize16, ysize16, pframes_count, row0, row1, stream=0):
        self._chk(self._L.m2v_strip_begin(self._h, xsize16, ysize16, pframes_count, d_frames_ptr, nframes, row0, row1,
                                          stream), "m2v_strip_begin")
        steps, hb = ctypes.c_int(0), ctypes.c_size_t(0)
        self._chk(self._L.m2v_strip_info(self._h, ctypes.byref(steps), ctypes.byref(hb)), "m2v_strip_info")
        return steps.value, hb.value

    def strip_step(self, j, send_up_ptr, send_down_ptr):
        return self._chk(self._L.m2v_strip_step(self._h, j, send_up_ptr, send_down_ptr), "m2v_strip_step")

    def strip_step_edges(self, j, send_up_ptr, send_down_ptr):
        return self._chk(self._L.m2v_strip_step_edges(self._h, j, send_up_ptr, send_down_ptr), "m2v_strip_step_edges")

    def strip_step_interior(self, j):
        self._chk(self._L.m2v_strip_step_interior(self._h, j), "m2v_strip_step_interior")

    def strip_halo_in(self, j, from_up_ptr, from_down_ptr):
        self._chk(self._L.m2v_strip_halo_in(self._h, j, from_up_ptr, from_down_ptr), "m2v_strip_halo_in")

    def strip_finish(self, d_strip_ptr, cap, nframes):
        off = np.zeros(nframes + 1, np.uint64)
        self._chk(self._L.m2v_strip_finish(self._h, d_strip_ptr, cap, off.ctypes.data), "m2v_strip_finish")
        return off

    def strip_finish_async(self, d_strip_ptr, cap):
        self._chk(self._L.m2v_strip_finish_async(self._h, d_strip_ptr, cap), "m2v_strip_finish_async")

    def strip_offsets(self, nframes):
        off = np.zeros(nframes + 1, np.uint64)
        self._chk(self._L.m2v_strip_offsets(self._h, off.ctypes.data), "m2v_strip_offsets")
        return off

    def strip_encode(self, comm, rank, world, d_frames_ptr, nframes, xsize16, ysize16, pframes_count, d_out_ptr=None, cap=0, dst=0, stream=0):
        """m2v_strip_encode: this rank's strip of one sequence, exchange included, in one native call.  `comm`: a StripComm
        (None for world == 1).  Returns the stream's byte count on rank `dst`, 0 elsewhere."""
        n = ctypes.c_size_t(0)
        self._chk(self._L.m2v_strip_encode(self._h, comm.handle if comm is not None else None, rank, world, dst, xsize16, ysize16,
                                           pframes_count, d_frames_ptr, nframes, d_out_ptr, cap, ctypes.byref(n), stream), "m2v_strip_encode")
        return n.value

    def strip_encode_begin(self, comm, rank, world, d_frames_ptr, nframes, xsize16, ysize16, pframes_count, d_out_ptr=None, cap=0, dst=0, stream=0):
        """m2v_strip_encode_begin: the sequence's GOP steps and this strip's slices are enqueued, nothing is waited for.  Two handles
        (a peer communicator each, over ONE base communicator) taking turns from one thread keep two strip sequences in flight."""
        self._chk(self._L.m2v_strip_encode_begin(self._h, comm.handle if comm is not None else None, rank, world, dst, xsize16, ysize16,
                                                 pframes_count, d_frames_ptr, nframes, d_out_ptr, cap, stream), "m2v_strip_encode_begin")

    def strip_encode_end(self):
        """m2v_strip_encode_end: the sizes all-gather, the one host wait, the strips to the output rank, the assembly there.
        Returns the stream's byte count on the output rank, 0 elsewhere."""
        n = ctypes.c_size_t(0)
        self._chk(self._L.m2v_strip_encode_end(self._h, ctypes.byref(n)), "m2v_strip_encode_end")
        return n.value

    def strip_stats(self):
        """-> dict of the last strip_encode: steps, host_us_per_step, and (option profile) halo_total / halo_exposed / gather in ms"""
        v = [ctypes.c_double(0) for _ in range(5)]
        steps = self._chk(self._L.m2v_strip_stats(self._h, *[ctypes.byref(x) for x in v]), "m2v_strip_stats")
        return {"steps": steps, "halo_total": v[0].value, "halo_exposed": v[1].value, "gather": v[2].value, "host_us_per_step": v[3].value,
                "comm_us_per_step": v[4].value, "host_us_per_step_outside_comm": v[3].value - v[4].value}

    def strip_last_form(self):
        """how the last strip_encode ran its GOP steps: "calls", "graph" or "peer" (m2v_strip_last_form)"""
        return ("calls", "graph", "peer")[self._chk(self._L.m2v_strip_last_form(self._h), "m2v_strip_last_form")]

    def strip_graph_stats(self):
        """-> dict: was the last strip_encode launched as a recorded hipGraph, how many recordings / launches so far, and whether
        recording has failed on this handle (the sequence is then enqueued call by call)"""
        v = [ctypes.c_int(0) for _ in range(3)]
        broken = self._chk(self._L.m2v_strip_graph_stats(self._h, *[ctypes.byref(x) for x in v]), "m2v_strip_graph_stats")
        return {"last_call_was_graph": bool(v[0].value), "recordings": v[1].value, "launches": v[2].value, "broken": bool(broken)}

    def strip_assemble(self, strip_ptrs, frame_offs, nframes, d_out_ptr, cap, xsize16, ysize16, pframes_count, stream=0):
        n = len(strip_ptrs)
        ptrs = (ctypes.c_void_p * n)(*strip_ptrs)
        offs = [np.ascontiguousarray(o, np.uint64) for o in frame_offs]
        optrs = (ctypes.c_void_p * n)(*[o.ctypes.data for o in offs])
        out = ctypes.c_size_t(0)
        self._chk(self._L.m2v_strip_assemble(self._h, xsize16, ysize16, pframes_count, nframes, n, ptrs, optrs, d_out_ptr,
                                             cap, ctypes.byref(out), stream), "m2v_strip_assemble")
        return out.value

    def kernel_stats(self, kernel):
        ms, units = ctypes.c_double(0), ctypes.c_double(0)
        n = self._chk(self._L.m2v_kernel_stats(self._h, kernel, ctypes.byref(ms), ctypes.byref(units)), "m2v_kernel_stats")
        return n, ms.value, units.value

    def debug_read(self, what, nbytes, dtype):
        buf = np.zeros(nbytes, np.uint8)
        n = self._chk(self._L.m2v_debug_read(self._h, what, buf.ctypes.data, nbytes), "m2v_debug_read")
        return buf[:n].view(dtype)


class StripComm:
    """The exchange between the strips of config c5 (include/m2v_mi355x.h, csrc/m2v_comm.hpp): RCCL between processes, or
    mailboxes between the threads of one process."""

    def __init__(self, handle, kind, world):
        self.handle, self.kind, self.world = handle, kind, world

    @classmethod
    def rccl(cls, rank, world, device, dist=None, init_timeout=None):
        """Collective over `dist` (an initialised torch.distributed of any backend, used ONLY to hand rank 0's ncclUniqueId to
        the others); afterwards the data path talks to librccl directly.

        Rank 0 broadcasts (status, id) whatever happened: when librccl cannot produce an id there, EVERY rank raises here,
        together, and nobody is left waiting in the broadcast.  ncclCommInitRank itself blocks until all ranks have arrived; a rank
        that cannot get there (its own librccl missing) would leave the others inside it, so with `init_timeout` (seconds) a rank
        still inside after that long ends its process with exit code 70 - a launcher that watches its ranks (bench.py) then tears
        the job down instead of hanging."""
        L = lib()
        status, ident = 128, None
        if rank == 0:
            buf = ctypes.create_string_buffer(128)
            status = L.m2v_comm_unique_id(buf, 128)
            ident = buf.raw if status == 128 else L.m2v_comm_last_error().decode()
        if world > 1:
            box = [(status, ident)]
            dist.broadcast_object_list(box, src=0)
            status, ident = box[0]
        if status != 128:
            raise M2VError("m2v_comm_unique_id failed on rank 0 (%d): %s" % (status, ident))
        err = ctypes.c_int(0)
        done = threading.Event()
        if init_timeout:
            def watchdog():
                if not done.wait(init_timeout):
                    sys.stderr.write("m2v: rank %d still inside m2v_comm_init_rccl after %.0f s (another rank never arrived?): giving up\n"
                                     % (rank, init_timeout))
                    sys.stderr.flush()
                    os._exit(70)
            threading.Thread(target=watchdog, daemon=True).start()
        try:
            h = L.m2v_comm_init_rccl(ident, rank, world, device, ctypes.byref(err))
        finally:
            done.set()
        if not h:
            raise M2VError("m2v_comm_init_rccl failed (%d): %s" % (err.value, L.m2v_comm_last_error().decode()))
        return cls(h, "rccl", world)

    @classmethod
    def local(cls, world, debug=False):
        """debug=True: made by the -DM2V_DEBUG library (for handles of that library: a communicator and its users come from ONE library)"""
        L = lib(debug)
        err = ctypes.c_int(0)
        h = L.m2v_comm_init_local(world, ctypes.byref(err))
        if not h:
            raise M2VError("m2v_comm_init_local failed (%d): %s" % (err.value, L.m2v_comm_last_error().decode()))
        c = cls(h, "local", world)
        c._debug = debug
        return c

    @classmethod
    def solo(cls, world, rccl=False, debug=False):
        """timing aid (tools/strip_solo.py): one rank of `world` alone on its GPU; the output is NOT a valid stream.
        rccl=True: the rows travel through a 1-rank RCCL communicator (ncclSend / ncclRecv to itself) instead of device copies"""
        L = lib(debug)
        err = ctypes.c_int(0)
        h = (L.m2v_comm_init_solo_rccl if rccl else L.m2v_comm_init_solo)(world, ctypes.byref(err))
        if not h:
            raise M2VError("m2v_comm_init_solo%s failed (%d): %s" % ("_rccl" if rccl else "", err.value, L.m2v_comm_last_error().decode()))
        c = cls(h, "solo-rccl" if rccl else "solo", world)
        c._debug = debug
        return c

    @classmethod
    def callbacks(cls, world, halo, allgather_u64, gather, debug=False):
        """The exchange supplied by the caller (m2v_comm_init_callbacks).  The three Python callables get the C arguments of
        m2v_comm_callbacks without `user` - device addresses as ints, the HIP stream as an int - and return 0 for success; an exception
        is reported as failure.  The callback objects live as long as the communicator."""
        L = lib(debug)

        def guard(fn):
            def run(user, *a):
                try:
                    return int(fn(*a) or 0)
                except BaseException as ex:  # noqa: BLE001  (nothing may unwind into C)
                    sys.stderr.write("m2v: communicator callback failed: %r\n" % (ex,))
                    return 1
            return run
        cb = CommCallbacks(CommCallbacks.HALO(guard(halo)), CommCallbacks.ALLGATHER(guard(allgather_u64)), CommCallbacks.GATHER(guard(gather)), None)
        err = ctypes.c_int(0)
        h = L.m2v_comm_init_callbacks(world, ctypes.byref(cb), ctypes.byref(err))
        if not h:
            raise M2VError("m2v_comm_init_callbacks failed (%d): %s" % (err.value, L.m2v_comm_last_error().decode()))
        c = cls(h, "callbacks", world)
        c._keep, c._debug = cb, debug
        return c

    @classmethod
    def peer(cls, base, rank, device=0, halo_bytes=0, connect=True):
        """The peer transport on top of `base` (m2v_comm_init_peer): rows stored straight into the neighbours' landing blocks by the
        macroblock kernel.  connect=True: m2v_comm_peer_connect_all - collective over `base` (every rank of it makes this call).
        `base` stays alive as long as the result (close this one first)."""
        L = lib(getattr(base, "_debug", False))
        err = ctypes.c_int(0)
        h = L.m2v_comm_init_peer(base.handle, rank, device, halo_bytes, ctypes.byref(err))
        if not h:
            raise M2VError("m2v_comm_init_peer failed (%d): %s" % (err.value, L.m2v_comm_last_error().decode()))
        c = cls(h, L.m2v_comm_kind(h).decode(), base.world)
        c._base, c._debug = base, getattr(base, "_debug", False)
        if connect:
            r = L.m2v_comm_peer_connect_all(h)
            if r < 0:
                msg = L.m2v_comm_last_error().decode()
                c.close()
                raise M2VError("m2v_comm_peer_connect_all failed (%d): %s" % (r, msg))
        return c

    def peer_export(self):
        buf = ctypes.create_string_buffer(PEER_DESC_BYTES)
        r = lib(getattr(self, "_debug", False)).m2v_comm_peer_export(self.handle, buf, PEER_DESC_BYTES)
        if r < 0:
            raise M2VError("m2v_comm_peer_export failed (%d): %s" % (r, lib().m2v_comm_last_error().decode()))
        return buf.raw

    def peer_connect(self, desc_up, desc_down):
        r = lib(getattr(self, "_debug", False)).m2v_comm_peer_connect(self.handle, desc_up, desc_down)
        if r < 0:
            raise M2VError("m2v_comm_peer_connect failed (%d): %s" % (r, lib().m2v_comm_last_error().decode()))

    def peer_stats(self):
        """-> dict: sequences that ran in the peer form, waits that gave up, and whether the communicator has fallen back to its base for good"""
        a, b = ctypes.c_ulonglong(0), ctypes.c_ulonglong(0)
        r = lib(getattr(self, "_debug", False)).m2v_comm_peer_stats(self.handle, ctypes.byref(a), ctypes.byref(b))
        if r < 0:
            raise M2VError("m2v_comm_peer_stats: not a peer communicator")
        return {"peer_sequences": a.value, "giveups": b.value, "fell_back": bool(r)}

    def selftest(self, rank, d_send_ptr, d_recv_ptr, nbytes, stream=0):
        r = lib().m2v_comm_selftest(self.handle, rank, d_send_ptr, d_recv_ptr, nbytes, stream)
        if r < 0:
            raise M2VError("m2v_comm_selftest failed (%d): %s" % (r, lib().m2v_comm_last_error().decode()))

    def selftest_captured(self, rank, d_send_ptr, d_recv_ptr, nbytes, stream=0, launches=2):
        """the same pair recorded into a hipGraph and launched `launches` times (can this transport be part of a recorded strip sequence?)"""
        r = lib().m2v_comm_selftest_captured(self.handle, rank, d_send_ptr, d_recv_ptr, nbytes, stream, launches)
        if r < 0:
            raise M2VError("m2v_comm_selftest_captured failed (%d): %s" % (r, lib().m2v_comm_last_error().decode()))

    def close(self):
        if getattr(self, "handle", None):
            lib(getattr(self, "_debug", False)).m2v_comm_destroy(self.handle)
            self.handle = None
