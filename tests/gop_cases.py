"""A level per GOP (m2v_set_gop_levels, option "gop_bytes_max"): the clips, and what the encoder must produce for them - shared by
tests/test_gop_cases.py and tests/test_gpu_gop_levels.py.  GOPs are closed and the level appears only in the slice headers, so the
stream of a sequence with level q[k] in GOP k is a splice of the oracle's streams of the whole clip: its sequence header, then for
every k the bytes of GOP k cut from the stream at Q_LEVEL = q[k], then the end code and the final-word padding.  Everything here comes
from the oracle; nothing looks at what the library computes."""
import functools

import numpy as np

import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()

SEQ_HEADER_BYTES = 34
GOP_CODE, END_CODE = b"\x00\x00\x01\xb8", b"\x00\x00\x01\xb7"

# name -> synth.clip arguments.  64 x 64 is the module's minimum (smaller sizes clamp up); scene cuts every few frames keep the GOPs'
# sizes apart.  "c80" with pframes_count = 2 is the checked example of the feature's description (GOPs of 3, 3 and 2 frames).
CLIPS = {
    "c64": dict(W=64, H=64, n=7, index=5, scene_len=2),
    "c80": dict(W=80, H=64, n=8, index=3, scene_len=3),
    "c96": dict(W=96, H=64, n=12, index=7, scene_len=4),
}


@functools.lru_cache(maxsize=None)
def frames(name):
    c = CLIPS[name]
    a = M.synth.clip(c["W"], c["H"], c["n"], c["index"], scene_len=c["scene_len"])
    a.setflags(write=False)
    return a


_cache = {}


def encoded(frames, W, H, pf, q, VL=3, conformant=False, nbeats=None):
    """(stream, dumps) of the oracle for these frames at Q_LEVEL = q, computed once; nbeats: the stop comes after that many beats"""
    f = np.ascontiguousarray(frames, np.uint8)
    key = (hash(f.tobytes()), f.shape[0], W, H, pf, q, VL, conformant, nbeats)
    if key not in _cache:
        _cache[key] = orc.encode(f, W // 16, H // 16, pf, 6, 6, VL, q, dump=True, conformant=conformant, nbeats=nbeats)
    return _cache[key]


def clip_args(name, n=None):
    """(frames, W, H) of a named clip, its first n frames"""
    c = CLIPS[name]
    return frames(name)[:n or c["n"]], c["W"], c["H"]


def cut(stream):
    """a stream -> (the bytes in front of the first GOP header, [the bytes of every GOP]): a GOP runs from its group_start_code up to the
    next one or to the sequence_end_code"""
    at = []
    k = stream.find(GOP_CODE)
    while k >= 0:
        at.append(k)
        k = stream.find(GOP_CODE, k + 4)
    end = stream.rfind(END_CODE)
    assert at and end > at[-1] and not any(stream[end + 4:])
    at.append(end)
    return stream[:at[0]], [stream[a:b] for a, b in zip(at, at[1:])]


def finish(body):
    """the end code and the final-word padding: the stream leaves in 32-byte words, and a last word always follows (RTL:2932-2937)"""
    body += END_CODE
    return body + bytes((len(body) // 32 + 1) * 32 - len(body))


def ngops(nframes, pf):
    return -(-nframes // (pf + 1))


def per_gop(levels, count):
    """a schedule -> the level of each of `count` GOPs: entry min(k, len - 1)"""
    levels = list(levels)
    return [levels[min(k, len(levels) - 1)] for k in range(count)]


def splice(frames, W, H, pf, levels, **params):
    """the expected stream of the frames with GOP k at levels[min(k, len - 1)]; params: VL, conformant, nbeats"""
    lv = per_gop(levels, ngops(len(frames), pf))
    head, _ = cut(encoded(frames, W, H, pf, lv[0], **params)[0])
    return finish(head + b"".join(cut(encoded(frames, W, H, pf, q, **params)[0])[1][k] for k, q in enumerate(lv)))


def gop_sizes(frames, W, H, pf, **params):
    """[4][nGOP]: the size of every GOP at levels 1..4"""
    return [[len(g) for g in cut(encoded(frames, W, H, pf, q, **params)[0])[1]] for q in (1, 2, 3, 4)]


def cap_levels(sizes, start, B):
    """the cap's rule: GOP k at the smallest level q >= start[k] whose size is <= B, searched upwards one level at a time, 4 if none is
    -> (levels, tries, over)"""
    levels, tries, over = [], [], []
    for k, q0 in enumerate(start):
        q = q0
        while q < 4 and sizes[q - 1][k] > B:
            q += 1
        levels.append(q)
        tries.append(q - q0 + 1)
        over.append(1 if sizes[q - 1][k] > B else 0)
    return levels, tries, over


def report(frames, W, H, pf, start, B, **params):
    """(the records m2v_gop_report must hand out, GOP_STAT_DTYPE; the levels): start = a schedule, or [Q_LEVEL]"""
    nf, count = len(frames), ngops(len(frames), pf)
    sizes = gop_sizes(frames, W, H, pf, **params)
    levels, tries, over = cap_levels(sizes, per_gop(start, count), B)
    r = np.zeros(count, M.GOP_STAT_DTYPE)
    for k in range(count):
        r[k] = (k, k * (pf + 1), min(pf + 1, nf - k * (pf + 1)), levels[k], sizes[levels[k] - 1][k], tries[k], over[k])
    return r, levels


def expected_qcodes(nframes, H, pf, levels):
    """Decoded.slice_qcodes of the stream with these levels: 1 << level for every slice of every picture"""
    lv = per_gop(levels, ngops(nframes, pf))
    return [[1 << lv[f // (pf + 1)]] * (H // 16) for f in range(nframes)]


# ---- the cases of the cap (tests/test_gop_cases.py shows what they reach; tests/test_gpu_gop_levels.py runs them) ----
SCHEDULE = [1, 4, 3]
# name -> clip, pframes_count, the handle's Q_LEVEL, schedule or None, B.  GOP 0 of "c80" is 3552 bytes at level 2.
CAP_CASES = {
    "b3500": ("c80", 2, 1, None, 3500),          # levels [3, 2, 1]: three different ones in one sequence, tries 3, 2, 1
    "b3552": ("c80", 2, 1, None, 3552),          # a cap equal to a GOP's exact size: it stays at 2
    "b3551": ("c80", 2, 1, None, 3551),          # ... and one byte less: it goes up
    "b800": ("c80", 2, 1, None, 800),            # tries 4; GOPs 0 and 1 are over even at 4
    "sched": ("c80", 2, 1, [2, 1, 3], 2100),     # start levels from a schedule, two of which the cap raises
    "q4": ("c64", 0, 4, None, 400),              # the handle at 4: nothing can go up (and nothing is waited for)
}


def cap_case(name):
    """-> dict(frames, W, H, pf, Q, start, B, records, levels, stream)"""
    clip, pf, Q, sched, B = CAP_CASES[name]
    f, W, H = clip_args(clip)
    start = sched or [Q]
    records, levels = report(f, W, H, pf, start, B)
    return dict(frames=f, W=W, H=H, pf=pf, Q=Q, sched=sched, B=B, records=records, levels=levels, stream=splice(f, W, H, pf, levels))
