"""The device decoder (m2v_decode_device): the streams it is tried on and what it must answer - shared by tests/test_dec_cases.py (CPU)
and tests/test_gpu_decode.py.  The definition is the expectation: decoder.decode(stream, quirks) - its frames, or its refusal (any
exception), plus the rule that a 00 00 01 prefix decoder.py did not read as a start code refuses the stream too.  Nothing here looks
at what the device computes.

host_lib(): the arithmetic of the device decoder (csrc/m2v_decode_kernels.hpp) and the serial harness tools/dec_host.hpp compiled for
the CPU with g++ - the same functions the kernels are thin loops over."""
import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

import desc_cases as DC
import entropy_clips as E
import recon_cases as R
import search_clips as SR
import transform_clips as T
from oracle import m2v_oracle_ctypes as orc

M = R.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ISO, MODULE = 0, 1
MODES = {"iso": ISO, "module": MODULE}
OK, SYNTAX, OVERFLOW = 0, -2, -3
LAYOUTS = R.LAYOUTS
GUARD, FILL = R.GUARD, R.FILL
STAT_FIELDS = ("es_bytes", "out_bytes", "frame_bytes", "err_offset", "pictures", "gops", "width", "height", "repeated_headers", "chains", "status")


class Stat(ctypes.Structure):
    """m2v_decode_stat (include/m2v_mi355x.h), 72 bytes"""
    _fields_ = [("es_bytes", ctypes.c_uint64), ("out_bytes", ctypes.c_uint64), ("frame_bytes", ctypes.c_uint64), ("err_offset", ctypes.c_uint64),
                ("pictures", ctypes.c_uint32), ("gops", ctypes.c_uint32), ("width", ctypes.c_uint32), ("height", ctypes.c_uint32),
                ("repeated_headers", ctypes.c_uint32), ("chains", ctypes.c_uint32), ("status", ctypes.c_int32), ("reserved", ctypes.c_uint32 * 3)]


# ---- the specification ----
def frames_of(dec, layout="i420"):
    """Decoded.frames -> [n, frame bytes] in `layout`, as m2v_decode_device must write them"""
    out = []
    for y, u, v in dec.frames:
        a, b = (u, v) if layout in ("i420", "nv12") else (v, u)
        c = np.concatenate([a.reshape(-1), b.reshape(-1)]) if layout in ("i420", "yv12") else np.stack([a, b], axis=2).reshape(-1)
        out.append(np.concatenate([y.reshape(-1), c]))
    return np.stack(out) if out else np.zeros((0, 0), np.uint8)


def units_read(dec):
    """the start codes decoder.decode read for what it returned"""
    mbh = (dec.height + 15) // 16
    return 3 * (1 + dec.repeated_headers) + len(dec.gops) + len(dec.pictures) * (2 + mbh) + 1


def prefixes(stream):
    n, at = 0, bytes(stream).find(b"\x00\x00\x01")
    while at >= 0:
        n += 1
        at = stream.find(b"\x00\x00\x01", at + 3)
    return n


def spec(stream, quirks):
    """-> (Decoded or None, 'raise' / 'prefix' / None): what the definition says of a stream"""
    stream = bytes(stream)
    try:
        d = M.decoder.decode(stream, quirks=quirks)
    except Exception:                       # every assert, ValueError and IndexError of decoder.py
        return None, "raise"
    if prefixes(stream) != units_read(d):
        return None, "prefix"
    return d, None


# ---- the host build ----
_HARNESS = r"""
#include "dec_host.hpp"
extern "C" long long dec_host_decode(const uint8_t *es, uint64_t n, int layout, int mode, uint8_t *out, uint64_t cap, dec_host::Record *rec)
{
    std::vector<uint8_t> frames;
    *rec = dec_host::decode(es, n, layout, mode, cap, frames);
    if (rec->status == 0 && !frames.empty()) memcpy(out, frames.data(), frames.size());
    return rec->status;
}
extern "C" unsigned dec_host_vlc(int which, unsigned w)
{
    using namespace m2v::dec;
    return which == 0 ? vlc_motion(w) : which == 1 ? vlc_cbp(w) : which == 2 ? vlc_dc_luma(w) : which == 3 ? vlc_dc_chroma(w) : vlc_ac(w);
}
extern "C" int dec_host_table(int which, int i) { return which ? m2v::dec::intra_weight(i) : (int)m2v::dec::scan_to_raster(i); }
extern "C" void dec_host_idct(int32_t *f, int mode)
{
    using namespace m2v::dec;
    for (int r = 0; r < 8; ++r) { int32_t a[8]; for (int k = 0; k < 8; ++k) a[k] = f[r * 8 + k]; idct_1d(a, true, mode); for (int k = 0; k < 8; ++k) f[r * 8 + k] = a[k]; }
    for (int c = 0; c < 8; ++c) { int32_t a[8]; for (int k = 0; k < 8; ++k) a[k] = f[k * 8 + c]; idct_1d(a, false, mode); for (int k = 0; k < 8; ++k) f[k * 8 + c] = a[k]; }
}
// a block of levels (raster; an intra block's [0] is its DC) -> F[64], as the reconstruction dequantises it
extern "C" void dec_host_dequant(const int32_t *q, int intra, int qcode, int mode, int32_t *f)
{
    using namespace m2v::dec;
    int32_t sum = 0;
    for (uint32_t i = 0; i < 64; ++i) { f[i] = intra && !i ? dequant_dc(q[0], mode) : dequant(q[i], i, intra != 0, 2 * qcode, mode); sum ^= f[i]; }
    if (mode == kIso && !(sum & 1)) f[63] = mismatch(f[63]);
}
extern "C" void dec_host_dequant_many(const int32_t *q, int count, int intra, int qcode, int mode, int32_t *f)
{
    for (int k = 0; k < count; ++k) dec_host_dequant(q + 64 * k, intra, qcode, mode, f + 64 * k);
}
extern "C" int dec_host_wrap(int pmv, int delta) { return m2v::dec::vector_wrap(pmv, delta); }
extern "C" unsigned dec_host_scan_tile(void) { return m2v::dec::kScanTile; }
"""

_host = None


def build_host(kernels_dir=None):
    """the harness above over tools/dec_host.hpp, compiled with g++ (no HIP) -> the library.  kernels_dir: a directory searched for
    m2v_decode_kernels.hpp in front of csrc (tests/test_dec_cases.py compiles altered copies of the header from a temporary one)"""
    d = tempfile.mkdtemp(prefix="m2v_dec_host_")
    src, so = os.path.join(d, "dec_host.cpp"), os.path.join(d, "libdec_host.so")
    with open(src, "w") as f:
        f.write(_HARNESS)
    inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
    first = ["-I", kernels_dir] if kernels_dir else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror"] + first + ["-I", inc, "-I", os.path.join(ROOT, "tools"), "-o", so, src])
    L = ctypes.CDLL(so)
    L.dec_host_decode.restype = ctypes.c_longlong
    L.dec_host_decode.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(Stat)]
    L.dec_host_vlc.restype = ctypes.c_uint
    L.dec_host_vlc.argtypes = [ctypes.c_int, ctypes.c_uint]
    L.dec_host_idct.argtypes = [ctypes.c_void_p, ctypes.c_int]
    L.dec_host_dequant.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.dec_host_dequant_many.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
    L.dec_host_scan_tile.restype = ctypes.c_uint
    return L


def host_lib():
    """tools/dec_host.hpp and csrc/m2v_decode_kernels.hpp as they stand"""
    global _host
    if _host is None:
        _host = build_host()
    return _host


def host_decode(stream, layout="i420", mode="module", cap=None, lib=None):
    """-> (frames [n, frame bytes] or None, the record as a dict); lib: a library of build_host() other than host_lib()"""
    stream = bytes(stream)
    room = (1 << 26) if cap is None else cap
    out = np.zeros(room, np.uint8)
    rec = Stat()
    (lib or host_lib()).dec_host_decode(stream, len(stream), M.LAYOUTS_420[layout], MODES[mode], out.ctypes.data, room, ctypes.byref(rec))
    r = {k: getattr(rec, k) for k in STAT_FIELDS}
    if r["status"] != OK:
        return None, r
    return out[:r["out_bytes"]].reshape(r["pictures"], -1).copy(), r


# ---- the valid streams ----
def _encode(clip, pf, VL, Q, conformant):
    clip = np.asarray(clip)
    return orc.encode(clip, clip.shape[3] // 16, clip.shape[2] // 16, pf, 7, 7, VL, Q, conformant=conformant)


@functools.lru_cache(maxsize=None)
def clip_stream(family, case, conformant):
    """the oracle's stream of a case of entropy_clips ("e"), search_clips ("s") or transform_clips ("t")"""
    if family == "e":
        clip, pf, VL, Q = E.cached_clip(*case)
    elif family == "s":
        (clip, pf), VL, Q = SR.cached_clip(*case), case[1], case[2]
    else:
        clip, pf, VL, Q = T.cached_clip(*case)
    return _encode(clip, pf, VL, Q, conformant)


def clip_cases():
    """(family, case) of the 22 entropy clips, the VL 3 search clips and the 42 transform clips"""
    return ([("e", c) for c in E.cases()] + [("s", c) for c in SR.cases() if c[1] == 3] + [("t", c) for c in T.cases()])


def clip_id(fc):
    family, case = fc
    return family + "-" + {"e": E.case_id, "s": SR.case_id, "t": T.case_id}[family](case)


@functools.lru_cache(maxsize=None)
def described():
    """a stream with repeated sequence headers in front of its second and third GOP, and a description that is not the module's"""
    c = R.case("chunks")
    pf = c["pf"]
    n = c["n"]
    firsts = [k for k in range(0, n, pf + 1)]
    d = DC.desc(frame_rate_code=5, aspect_ratio_information=3, bit_rate_400=123456, vbv_buffer_size_16k=77, video_format=2,
                colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1, repeat_headers=1)
    return DC.described(c["stream"], firsts, d)


@functools.lru_cache(maxsize=None)
def recon_streams():
    """name -> (stream, conformant, coded W, H, region or None, the oracle's recon dump) for every case of recon_cases.gpu_cases(), and the
    fit cases again with the true size in the header"""
    out = {}
    for name, c in R.gpu_cases().items():
        out[name] = dict(stream=c["stream"], conformant=bool(c.get("conformant", False)), W=c["W"], H=c["H"], region=None, recon=c["recon"])
        if c.get("region"):
            w, h = c["region"]
            out[name + "_true"] = dict(stream=M.set_header_size(c["stream"], w, h), conformant=False, W=c["W"], H=c["H"], region=(w, h), recon=c["recon"])
    return out


TWINS = ("unref", "ionly", "chunks", "conformant", "vl1q4", "g80", "g272")


@functools.lru_cache(maxsize=None)
def twin_streams():
    """name -> the stream of a case of recon_streams() in the other encoding (conformant where the case is plain, plain for "conformant"),
    for the cases that are one call of the oracle: the geometry cases, the fit cases (also with the true size in the header), and
    "described" - the described stream's twin.  "levels", "cap" and "starts" are spliced from several calls by gop_cases / scene_cases,
    which encode plain only; their GOPs are those of "chunks"-like clips, whose twins are here."""
    out = {}
    for name in TWINS:
        c = R.case(name)
        out[name] = orc.encode(c["frames"], c["W"] // 16, c["H"] // 16, c["pf"], *c["params"], conformant=not c.get("conformant", False))
    for w, h in R.FIT_SIZES:
        for kind in R.FIT_KINDS:
            c = R.fit_case(w, h, kind)
            s = orc.encode(R.F.planes(c["x"], w, h, kind), c["W"] // 16, c["H"] // 16, c["pf"], *c["params"], conformant=True)
            out["fit%dx%d_%s" % (w, h, kind)] = s
            out["fit%dx%d_%s_true" % (w, h, kind)] = M.set_header_size(s, w, h)
    c = R.case("chunks")
    d = DC.desc(frame_rate_code=5, aspect_ratio_information=3, bit_rate_400=123456, vbv_buffer_size_16k=77, video_format=2,
                colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1, repeat_headers=1)
    out["described"] = DC.described(out["chunks"], [k for k in range(0, c["n"], c["pf"] + 1)], d)
    return out


def twin_names():
    fit = ["fit%dx%d_%s" % (w, h, kind) for w, h in R.FIT_SIZES for kind in R.FIT_KINDS]
    return sorted(list(TWINS) + fit + [n + "_true" for n in fit] + ["described"])


def recon_names():
    """the names of recon_streams(), without encoding anything"""
    fit = ["fit%dx%d_%s" % (w, h, kind) for w, h in R.FIT_SIZES for kind in R.FIT_KINDS]
    return sorted(["unref", "ionly", "chunks", "conformant", "vl1q4", "g80", "g272", "levels", "cap", "starts"] + fit + [n + "_true" for n in fit])


def expected_from_dump(c, layout):
    """the frames the device must write for an entry of recon_streams(), from the oracle's dump"""
    return R.write_layout(c["recon"], c["W"], c["H"], layout, c["region"])


# ---- the small stream of the refusal tests: 32 x 32, one I and one P picture ----
class _Writer:
    """bits of slice data, most significant first"""
    def __init__(self):
        self.s = ""

    def put(self, value, width):
        assert 0 <= value < (1 << width)
        self.s += format(value, "0%db" % width) if width else ""

    def code(self, entry):
        self.put(entry[0], entry[1])

    def bytes(self):
        s = self.s + "0" * (-len(self.s) % 8)
        return int(s, 2).to_bytes(len(s) // 8, "big")


def _write_block(w, rng, t, intra, chroma):
    """one coded block: [DC size and differential,] a few run/level pairs - table codes and escapes -, end of block"""
    ac = {sym: (code, length) for code, length, sym in t["ac"]}
    if intra:
        diff = int(rng.randint(-60, 61))
        size = 0 if diff == 0 else int(abs(diff)).bit_length()
        w.code({sym: (code, length) for code, length, sym in t["dcc" if chroma else "dcy"]}[size])
        if size:
            w.put(diff if diff > 0 else diff + (1 << size) - 1, size)
    first, k = not intra, 1 if intra else 0
    for _ in range(int(rng.randint(1, 5))):
        run, lvl = int(rng.randint(0, 6)), int(rng.randint(1, 9)) * (1 if rng.randint(2) else -1)
        if k + run > 63:
            break
        if rng.randint(8) == 0:
            lvl *= 9                                          # no table code: an escape
        if first and run == 0 and abs(lvl) == 1:
            w.put(1, 1)
            w.put(lvl < 0, 1)
        elif (run, abs(lvl)) in ac:
            w.code(ac[(run, abs(lvl))])
            w.put(lvl < 0, 1)
        else:
            w.put(1, 6)
            w.put(run, 6)
            w.put(lvl & 0xFFF, 12)
        first, k = False, k + run + 1
    w.put(2, 2)


@functools.lru_cache(maxsize=None)
def small(seed=7):
    """A 32 x 32 stream of one I and one P picture (the oracle's smallest picture is 64 x 64): written bit by bit from decoder.py's
    tables with seeded content - intra, MC coded, MC not coded, table codes, escapes -, and accepted by decoder.decode in both modes."""
    t = M.decoder.iso_tables()
    rng = np.random.RandomState(seed)
    motion = {sym: (code, length) for code, length, sym in t["motion"]}
    cbps = {sym: (code, length) for code, length, sym in t["cbp"]}
    out = DC.seq_headers(32, 32, DC.MODULE) + b"\x00\x00\x01\xb8" + DC.time_code(0, 2)
    for n, ptype in enumerate((1, 2)):
        w = _Writer()
        for value, width in ((0x00000100, 32), (n, 10), (ptype, 3), (0xFFFF, 16)) + (((0, 1), (7, 3)) if ptype == 2 else ()) + ((0, 1),):
            w.put(value, width)
        out += w.bytes()
        w = _Writer()
        for value, width in ((0x000001B5, 32), (8, 4), (1, 4), (1, 4), (15, 4), (15, 4), (2, 2), (3, 2), (0, 1), (1, 1), (0, 1), (0, 1), (0, 1), (0, 1),
                             (0, 1), (1, 1), (1, 1), (0, 1)):
            w.put(value, width)
        out += w.bytes()
        for row in range(2):
            w = _Writer()
            w.put(0x00000101 + row, 32)
            w.put(4, 5)
            w.put(0, 1)
            pmv = [0, 0]
            for col in range(2):
                w.put(1, 1)
                kind = "intra" if ptype == 1 else ("coded", "coded", "not_coded", "intra")[(2 * row + col + seed) % 4]
                if ptype == 1:
                    w.put(1, 1)
                elif kind == "intra":
                    w.put(3, 5)
                else:
                    w.put(1, 1 if kind == "coded" else 3)
                    # a vector that stays inside: away from the picture's edge, at most 3 half samples
                    mv = [int(rng.randint(0, 4)) * (1 if col == 0 else -1), int(rng.randint(0, 4)) * (1 if row == 0 else -1)]
                    for c in range(2):
                        d = mv[c] - pmv[c]
                        w.code(motion[abs(d)])
                        if d:
                            w.put(d < 0, 1)
                    pmv = mv
                if kind == "intra":
                    pmv = [0, 0]
                cbp = 63 if kind == "intra" else 0 if kind == "not_coded" else int(rng.randint(1, 64))
                if kind == "coded":
                    w.code(cbps[cbp])
                for b in range(6):
                    if (cbp >> (5 - b)) & 1:
                        _write_block(w, rng, t, kind == "intra", b >= 4)
            out += w.bytes()
    out += b"\x00\x00\x01\xb7"
    out += bytes(-len(out) % 32)
    for quirks in (True, False):
        d = M.decoder.decode(out, quirks=quirks)
        assert [p["type"] for p in d.pictures] == [1, 2] and (d.width, d.height) == (32, 32) and prefixes(out) == units_read(d)
    return out


def first_slice(stream):
    return bytes(stream).find(b"\x00\x00\x01\x01")


def flip(stream, bit):
    b = bytearray(stream)
    b[bit >> 3] ^= 0x80 >> (bit & 7)
    return bytes(b)


def _units(stream):
    """[(offset, code)] of every start code"""
    out, at = [], stream.find(b"\x00\x00\x01")
    while at >= 0 and at + 3 < len(stream):
        out.append((at, stream[at + 3]))
        at = stream.find(b"\x00\x00\x01", at + 3)
    return out


@functools.lru_cache(maxsize=None)
def handmade():
    """name -> altered small stream; every one is refused by the definition"""
    s = small()
    u = _units(s)
    pos = {code: [a for a, c in u if c == code] for code in set(c for _, c in u)}
    h = {}
    b = bytearray(s)
    p0 = pos[0x00][0]
    b[p0 + 5] = (b[p0 + 5] & ~0x38) | (3 << 3)
    h["picture_type_3"] = bytes(b)
    b = bytearray(s)
    x = [a for a in pos[0xB5] if a > p0][0]                  # the first picture coding extension: intra_vlc_format is bit 5 of its 8th byte
    b[x + 7] |= 0x20
    h["intra_vlc_format_1"] = bytes(b)
    b = bytearray(s)
    b[pos[0x01][0] + 3], b[pos[0x02][0] + 3] = 2, 1
    h["slices_out_of_order"] = bytes(b)
    end = pos[0xB7][0]
    h["end_code_missing"] = s[:end] + bytes(len(s) - end)
    h["nonzero_after_end"] = s[:-1] + b"\x01"
    h["length_not_32"] = s + b"\x00"
    b = bytearray(s)
    b[p0 + 5] = (b[p0 + 5] & ~0x38) | (2 << 3)
    h["p_picture_first"] = bytes(b)
    return h


def truncations():
    s = small()
    return {"cut_in_slice": s[:first_slice(s) + 9], "cut_in_header": s[:40]}


@functools.lru_cache(maxsize=None)
def ionly_stream():
    """desc_cases.ionly(): 62 I pictures of 64 x 64, 248 slices - four blocks of the slice walk in one chunk"""
    frames, W, H = DC.ionly()
    return orc.encode(np.asarray(frames), W // 16, H // 16, 0, 7, 7, 3, 2)


@functools.lru_cache(maxsize=None)
def two_bad_slices():
    """-> (stream, offset of the earlier bad slice): ionly_stream() with extra_bit_slice set in slice 21 (picture 5) and in slice 162
    (picture 40), which the slice walk meets in different blocks: the earlier one is what err_offset names, whichever is walked first.
    (The altered byte holds a bit that is not its lowest, so no start-code prefix appears.)"""
    s = bytearray(ionly_stream())
    slices = [a for a, c in _units(bytes(s)) if 1 <= c <= 0xAF]
    assert len(slices) == 248
    for k in (162, 21):
        s[slices[k] + 4] |= 0x04
    return bytes(s), slices[21]


def altered(seed=1, flips=400, edits=100):
    """[(name, stream)]: seeded single-bit flips in slice data, truncations and byte insertions"""
    s = small()
    rng = np.random.RandomState(seed)
    lo, hi = 8 * (first_slice(s) + 4), 8 * s.find(b"\x00\x00\x01\xb7")
    out = [("flip%d" % bit, flip(s, int(bit))) for bit in rng.randint(lo, hi, size=flips)]
    for k in range(edits):
        at = int(rng.randint(lo // 8, hi // 8))
        if k % 2:
            out.append(("cut%d" % at, s[:at]))
        else:
            out.append(("ins%d" % at, s[:at] + bytes([int(rng.randint(0, 256))]) + s[at:]))
    return out


# ---- the scan's tile: noise clips whose seeds make the oracle's streams meet tile_census (test_scan_tile_streams asserts it) ----
TILE_SEEDS = ((0, 40, 3), (8, 40, 3), (16, 40, 3), (33, 40, 3), (42, 40, 3), (1013, 16, 0))      # (seed, frames, pframes_count)


def noise_clip(seed, n, amp=6):
    rng = np.random.RandomState(seed)
    base = rng.randint(64, 192, size=(1, 3, 64, 64))
    return np.clip(base + rng.randint(-amp, amp + 1, size=(n, 3, 64, 64)), 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def tile_streams(conformant=False):
    """the oracle's streams of the noise clips, 64 x 64, with a repeated sequence header in front of every GOP but the first (the seeds
    are chosen for the plain encoding; the conformant one is the same clips' other encoding)"""
    return tuple(DC.described(orc.encode(noise_clip(seed, n), 4, 4, pf, 7, 7, 3, 2, conformant=conformant), DC.cadence(n, pf), DC.desc(repeat_headers=1))
                 for seed, n, pf in TILE_SEEDS)


UNIT_KINDS = ("sequence", "sequence_ext", "display_ext", "gop", "picture", "picture_ext", "slice", "end")


def unit_kinds(stream):
    """[(offset, kind)] of every start code: a B5 is what the codes in front of it make it, as in decoder.py"""
    out, codes = [], []
    for a, c in _units(stream):
        if c == 0xB5:
            kind = ("sequence_ext" if codes[-1:] == [0xB3] else "picture_ext" if codes[-1:] == [0x00] else
                    "display_ext" if codes[-2:] == [0xB3, 0xB5] else "")
        else:
            kind = {0xB3: "sequence", 0xB8: "gop", 0x00: "picture", 0xB7: "end"}.get(c, "slice" if 1 <= c <= 0xAF else "")
        codes.append(c)
        out.append((a, kind))
    return out


def tile_census(streams, T, by_kind=False):
    """what the streams' start codes do at the multiples of T: the set of "T-3", "T-2", "T-1", "T" (a start code begins there) and of
    "slice", "picture", "sequence" (such a unit begins in one tile and ends in the next).
    by_kind: instead the set of (kind of unit, where it begins) over UNIT_KINDS, where = "T-3" .. "T" as above, "16-3" .. "16" (so far
    from a multiple of 16 that is not within 16 bytes of a multiple of T), and of ("tile", k) for every tile k a start code begins in"""
    got = set()
    for s in streams:
        u = _units(s)
        if by_kind:
            for a, kind in unit_kinds(s):
                if a >= T - 3:
                    got.add((kind, {T - 3: "T-3", T - 2: "T-2", T - 1: "T-1", 0: "T"}.get(a % T, "")))
                if 16 <= (a + 3) % T and (a + 3) % T < T - 16:
                    got.add((kind, {13: "16-3", 14: "16-2", 15: "16-1", 0: "16"}.get(a % 16, "")))
                got.add(("tile", a // T))
            continue
        for k, (a, c) in enumerate(u):
            end = u[k + 1][0] if k + 1 < len(u) else len(s)
            if a >= T - 3:
                got |= {{T - 3: "T-3", T - 2: "T-2", T - 1: "T-1", 0: "T"}.get(a % T, "")}
            if a // T != (end - 1) // T:
                got.add("slice" if 1 <= c <= 0xAF else "picture" if c == 0 else "sequence" if c == 0xB3 else "")
    if by_kind:
        return {g for g in got if g[1] != "" and g[0] != ""}
    return got - {""}


def pack_streams(items):
    """[(stream, mode)] -> the file tools/dec_host_check reads: count, then per stream mode, length (uint32 / uint64, little endian), bytes"""
    import struct
    out = [struct.pack("<I", len(items))]
    for stream, mode in items:
        out += [struct.pack("<IQ", MODES[mode], len(stream)), bytes(stream)]
    return b"".join(out)
