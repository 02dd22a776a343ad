"""A batch of sequences in one resident call (m2v_set_sequences): the clips, the lists, and what the encoder must produce for them -
shared by tests/test_seq_cases.py and tests/test_gpu_sequences.py.  The definition is the expectation: the bytes at
[off[b], off[b + 1]) are the oracle's stream of clip b encoded alone, so the expected output is the concatenation of
oracle.encode(clip_b), and the offsets are the running sum of those streams' lengths.  Everything here comes from the oracle (and, for a
level schedule, a description, the statistics and the reconstruction, from the case modules that already derive those from the oracle
per sequence); nothing looks at what the library computes."""
import functools

import numpy as np

import desc_cases as D
import gop_cases as G
import recon_cases as R
import stats_cases as S

M = G.M
END_CODE = G.END_CODE

# The list of the parity cases: four one-frame sequences first (a chunk of four frames in which every frame is a sequence), then 3, 9,
# 2, 10 and 4 frames.  Sequence ends (exclusive) at 1, 2, 3, 4, 7, 16, 18, 28, 32.
MIXED = (1, 1, 1, 1, 3, 9, 2, 10, 4)
FIVES = (5,) * 6
CHUNKS = (96, 4, 5)            # "batch_frames": the default (one chunk holds the batch), and two grids that cut the sequences
# name -> coded size, list, pframes_count, the seed of the material
PARITY = {
    "mixed_pf2": dict(W=96, H=64, lengths=MIXED, pf=2, seed=41),
    "mixed_pf3": dict(W=160, H=128, lengths=MIXED, pf=3, seed=42),
    "fives_pf4": dict(W=64, H=64, lengths=FIVES, pf=4, seed=43),
}

# Clips whose bytes in front of the sequence_end_code leave these remainders mod 32 - what the final-word rule turns on: with 28 the end
# code fills the word exactly and a whole extra zero word leaves (RTL:2932-2937).  Found by a seed search on the CPU over
# synth.clip(64, 64, n, seed, scene_len=2) at pframes_count 1, Q_LEVEL 2, VECTOR_LEVEL 3, seeds 300 ..: remainder -> (seed, frames).
REMAINDERS = {0: (300, 2), 28: (309, 2), 27: (312, 1), 29: (324, 1), 31: (327, 1)}
REM_PF = 1


def lengths_offsets(streams):
    off = [0]
    for s in streams:
        off.append(off[-1] + len(s))
    return off


def split(frames, lengths):
    """the frames of a call -> the clips of the list"""
    assert sum(lengths) == len(frames)
    out, at = [], 0
    for n in lengths:
        out.append(frames[at:at + n])
        at += n
    return out


def front_bytes(stream):
    """bytes in front of the sequence_end_code"""
    B = stream.rfind(END_CODE)
    assert B > 0 and not any(stream[B + 4:])
    return B


@functools.lru_cache(maxsize=None)
def material(W, H, n, seed):
    """n frames [n, 3, H, W] with a scene cut every 7 frames, so that clips cut from it differ"""
    a = M.synth.clip(W, H, n, seed, scene_len=7)
    a.setflags(write=False)
    return a


def streams(frames, lengths, W, H, pf, Q=2, **params):
    """the oracle's stream of every clip alone; params: VL, conformant"""
    return [G.encoded(c, W, H, pf, Q, **params)[0] for c in split(frames, lengths)]


def expected(frames, lengths, W, H, pf, Q=2, **params):
    """-> (the bytes the call must write, the offsets off[0 .. n])"""
    s = streams(frames, lengths, W, H, pf, Q, **params)
    return b"".join(s), lengths_offsets(s)


def records(lengths, offsets, pf):
    """what m2v_sequence_report must hand out"""
    r = np.zeros(len(lengths), M.SEQUENCE_STAT_DTYPE)
    f0 = 0
    for b, n in enumerate(lengths):
        r[b] = (offsets[b], offsets[b + 1] - offsets[b], f0, n, G.ngops(n, pf), 0)
        f0 += n
    return r


@functools.lru_cache(maxsize=None)
def parity(name):
    """-> dict(frames, W, H, lengths, pf)"""
    c = dict(PARITY[name])
    c["lengths"] = list(c["lengths"])
    c["frames"] = material(c["W"], c["H"], sum(c["lengths"]), c["seed"])
    return c


@functools.lru_cache(maxsize=None)
def remainder_case():
    """-> dict(frames, W, H, lengths, pf, remainders): the five clips of REMAINDERS in one batch, in the order 28, 0, 27, 31, 29"""
    order = (28, 0, 27, 31, 29)
    clips = [M.synth.clip(64, 64, REMAINDERS[r][1], REMAINDERS[r][0], scene_len=2) for r in order]
    f = np.ascontiguousarray(np.concatenate(clips))
    f.setflags(write=False)
    return dict(frames=f, W=64, H=64, lengths=[len(c) for c in clips], pf=REM_PF, remainders=list(order))


def situations(lengths, chunk):
    """what a chunk grid of `chunk` frames does to the list: a set of names"""
    out, f0, total = set(), 0, sum(lengths)
    for n in lengths:
        last = f0 + n - 1
        if n == 1:
            out.add("one_frame")
        if (last + 1) % chunk == 0 and last + 1 != total:
            out.add("ends_on_chunk_last")
        if last % chunk == 0 and n > 1:
            out.add("ends_on_chunk_first")
        if last % chunk not in (0, chunk - 1) and last + 1 != total:
            out.add("ends_inside")
        if last // chunk - f0 // chunk >= 2:
            out.add("spans_three_chunks")
        f0 += n
    starts = set(np.cumsum([0] + list(lengths))[:-1].tolist())
    for c0 in range(0, total - chunk + 1, chunk):
        if all(f in starts for f in range(c0, c0 + chunk)):
            out.add("every_frame_a_sequence")
    return out


ALL_SITUATIONS = {"one_frame", "ends_on_chunk_last", "ends_on_chunk_first", "ends_inside", "spans_three_chunks", "every_frame_a_sequence"}


# ---- the scan's own trip points: I-only one-frame sequences of 64 x 64 (4 slices a frame) in ONE chunk.  k_seq_scan's constants
# (csrc/m2v_seq_kernels.hpp): 1024 threads, 4 cached items a thread - more than 1024 items give a thread two, more than 4096 send it
# past its cached ones, more than 1024 sequences give a thread two of those and send their hand-over from LDS to memory.  256 frames are
# exactly 1024 items: just below the first.
TRIP_DISTINCT = 8
TRIP_COUNTS = {"below": 256, "above_all": 1100}


@functools.lru_cache(maxsize=None)
def trip_frames():
    a = M.synth.clip(64, 64, TRIP_DISTINCT, 77, scene_len=1)
    a.setflags(write=False)
    return a


def trip_case(name):
    """-> dict(frames [n, 3, 64, 64], lengths [1] * n, pf 0, stream, offsets): the frames cycle through TRIP_DISTINCT pictures"""
    n = TRIP_COUNTS[name]
    base = trip_frames()
    one = [G.encoded(base[k:k + 1], 64, 64, 0, 2)[0] for k in range(TRIP_DISTINCT)]
    idx = [(k * 5 + k // TRIP_DISTINCT) % TRIP_DISTINCT for k in range(n)]
    s = [one[k] for k in idx]
    return dict(frames=np.ascontiguousarray(base[idx]), W=64, H=64, lengths=[1] * n, pf=0, stream=b"".join(s), offsets=lengths_offsets(s))


# ---- composition: one case each, every expectation per clip ----
COMP = dict(W=96, H=64, lengths=[2, 5, 1, 4], pf=2, seed=44)


@functools.lru_cache(maxsize=None)
def comp():
    c = dict(COMP)
    c["frames"] = material(c["W"], c["H"], sum(c["lengths"]), c["seed"])
    return c


def levels_expected(levels):
    """a level schedule goes by the GOP's ordinal inside its own sequence: gop_cases' splice, per clip"""
    c = comp()
    s = [G.splice(x, c["W"], c["H"], c["pf"], levels) for x in split(c["frames"], c["lengths"])]
    return b"".join(s), lengths_offsets(s)


def desc_expected(d):
    """a description: desc_cases' rewrite, per clip - every clip's time codes start at 0"""
    c = comp()
    s = [D.described(G.encoded(x, c["W"], c["H"], c["pf"], 2)[0], D.cadence(len(x), c["pf"]), d) for x in split(c["frames"], c["lengths"])]
    return b"".join(s), lengths_offsets(s)


def stats_expected(**params):
    """option "stats": the records of each clip alone, in batch order"""
    c = comp()
    return np.concatenate([S.records(G.encoded(x, c["W"], c["H"], c["pf"], 2, **params)[1], c["W"], c["H"], c["pf"])
                           for x in split(c["frames"], c["lengths"])])


def recon_expected(layout):
    """m2v_set_recon_out: frame n of the call at n * frame_bytes - the pictures of each clip alone, one behind the other"""
    c = comp()
    rec = np.concatenate([G.encoded(x, c["W"], c["H"], c["pf"], 2)[1]["recon"] for x in split(c["frames"], c["lengths"])])
    return R.write_layout(rec, c["W"], c["H"], layout)
