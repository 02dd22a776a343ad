"""One model of a call with every setting at once: what a resident call (or a sequence on the port path) must hand back for any legal
combination of input kind, frame size and header mode, "conformant", a level schedule or the byte cap, a GOP list and / or the
scene-cut detector, a stream description, a batch of sequences, "stats", a reconstruction buffer, a container buffer, any chunking and
either entry - shared by tests/test_compose_cases.py (CPU) and tests/test_gpu_compose.py.

A call is a dict of the factors below (FACTORS names them and their levels).  expected(call) composes, in the order the README states,
what the older case modules already derive from the oracle for one feature each: source -> planar 4:4:4 (fit_cases), clips
(seq_cases.split), the GOP layout per clip (scene_cases.layout), every GOP as GOP 0 of the oracle's stream of its own frames encoded
alone at the level of the schedule or of the cap's rule (gop_cases), time codes and sequence headers (desc_cases), the stream tail
(gop_cases.finish), statistics and reconstruction from the dump of the same encode (stats_cases, recon_cases) and the CPU muxers over
every clip's stream (mux_cases).  Nothing the device computes enters it.

legal(call) is the literal table of what may be set together; pairs() is a seeded greedy covering array over the factors in which every
legal pair of levels occurs; maximal() holds the three largest legal sets; session() a dozen calls for one handle.
check(got, want) is the one comparison - byte for byte, integer for integer - and names the item that differs.

Measured by tests/test_compose_cases.py (the figures its tests print): pairs() has 27 rows (772 legal pairs of levels), port_pairs() 19 (300)."""
import functools
import random

import numpy as np

import desc_cases as D
import fit_cases as F
import gop_cases as G
import mux_cases as X
import recon_cases as R
import scene_cases as SC
import seq_cases as Q
import stats_cases as S

M = G.M

N, SCENE_LEN, CLIP_INDEX = 12, 5, 61          # the frames of every call: synth.clip(..., scene_len=5), scenes change at frames 5 and 10
SCHEDULE = (1, 4, 3)
LIST = (3, 8)                                 # (with either pframes_count both scene changes stay off the cadence)
SEQS = (2, 5, 1, 4)
DESC = dict(frame_rate_code=4, colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1, aspect_ratio_information=3,
            bit_rate_400=20000, vbv_buffer_size_16k=112)
SENTINEL = X.SENTINEL                         # the stream and the container buffer
FILL, GUARD = R.FILL, R.GUARD                 # the reconstruction buffer

PLAIN_GEOM, FIT_MODULE, FIT_TRUE, SMALL_GEOM = (96, 64, None), (100, 70, "module"), (100, 70, "true"), (64, 64, None)
FACTORS = (
    ("geom", (PLAIN_GEOM, FIT_MODULE, FIT_TRUE)),         # (w, h, header mode or None: no size set)
    ("pf", (2, 3)),
    ("kind", ("444", "i420", "nv12", "rgb24", "rgbp")),   # (rgbp goes with the bt709 matrix, rgb24 with bt601)
    ("conformant", (0, 1)),
    ("vlq", ((3, 2), (1, 4))),                            # (VECTOR_LEVEL, Q_LEVEL) of the handle
    ("rate", (None, "sched", "cap")),                     # the schedule SCHEDULE, or the cap B = cap_bytes(call)
    ("layout", (None, "list", "cut", "both")),            # the list LIST, the detector at T = threshold(call)
    ("desc", (None, "fields", "repeat")),                 # DESC, and DESC with repeat_headers
    ("seqs", (None, "batch")),                            # SEQS
    ("stats", (0, 1)),
    ("recon", (None, "i420", "nv12")),
    ("mux", (None, "ts", "ps")),
    ("chunk", (96, 4, 5)),                                # "batch_frames"
    ("split", (1, 3)),                                    # "split_streams"
    ("entry", ("block", "begin")),
)
# the port path (push_frames / encode()): the settings it accepts
PORT_FACTORS = (
    ("geom", (PLAIN_GEOM, FIT_MODULE, FIT_TRUE)),
    ("pf", (2, 3)),
    ("kind", ("444", "i420", "nv12", "rgb24", "rgbp")),
    ("conformant", (0, 1)),
    ("vlq", ((3, 2), (1, 4))),
    ("rate", (None, "sched")),
    ("layout", (None, "list")),
    ("desc", (None, "fields", "repeat")),
    ("stats", (0, 1)),
    ("chunk", (96, 4, 5)),
)
OFF = dict(geom=PLAIN_GEOM, pf=2, kind="444", conformant=0, vlq=(3, 2), rate=None, layout=None, desc=None, seqs=None, stats=0, recon=None,
           mux=None, chunk=96, split=2, entry="block")           # a handle with nothing set (split_streams' default is 2)
# the settings a handle keeps between calls (the others are arguments of the call or fixed at creation)
SETTINGS = ("size", "conformant", "rate", "layout", "desc", "seqs", "stats", "recon", "mux", "chunk", "split")

# what may not be set together (include/m2v_mi355x.h, the README): pairs of (factor, level)
EXCLUDED = (
    (("seqs", "batch"), ("layout", "list")), (("seqs", "batch"), ("layout", "cut")), (("seqs", "batch"), ("layout", "both")),
    (("seqs", "batch"), ("rate", "cap")),
    (("rate", "cap"), ("layout", "list")), (("rate", "cap"), ("layout", "cut")), (("rate", "cap"), ("layout", "both")),
)
# ... and what the port path refuses: the cap, the detector, sequences, the reconstruction buffer, the container buffer
PORT_EXCLUDED = (("rate", "cap"), ("layout", "cut"), ("layout", "both"), ("seqs", "batch"), ("recon", "i420"), ("recon", "nv12"),
                 ("mux", "ts"), ("mux", "ps"))


def call(**levels):
    """a call: a handle with nothing set, with these factors replaced"""
    assert set(levels) <= set(OFF) | {"material"}, levels
    return dict(OFF, **levels)


def legal(c):
    """the literal table: may the settings of this call be set together?  (strips refuse everything and are no factor here)"""
    if c.get("strips"):
        return False
    cap = c["rate"] == "cap" or (isinstance(c["rate"], tuple) and c["rate"][0] == "cap")
    detector = c["layout"] in ("cut", "both") or (isinstance(c["layout"], tuple) and c["layout"][2])
    if c["seqs"] and (c["layout"] or cap):
        return False                                      # sequences refuse the GOP list, the detector and the cap
    if cap and c["layout"]:
        return False                                      # the cap refuses the list and the detector
    if cap and c["pf"] + 1 > c["chunk"]:
        return False                                      # the cap needs whole GOPs in a chunk (M2V_E_PARAM, not a refusal of a pair)
    if c["entry"] == "port" and (cap or detector or c["seqs"] or c["recon"] or c["mux"]):
        return False                                      # the port path refuses the cap, the detector, sequences, both buffers
    return True


def name_of(c, factors=FACTORS):
    """the levels of a call, spelled out: the id of its test case"""
    def one(f, v):
        if f == "geom":
            return "%dx%d%s" % (v[0], v[1], "" if v[2] is None else v[2][0])
        if f == "vlq":
            return "vl%dq%d" % v
        if f in ("kind", "entry"):
            return str(v)
        return "%s%s" % (f, 0 if v is None else v)
    return "-".join(one(f, c[f]) for f, _ in factors)


# ---- rows ----
def covering(factors, base, seed, tries=30):
    """a deterministic greedy covering array: rows (calls) over `factors`, the other factors as in `base`, each legal, in which every
    pair of levels that occurs in some legal row occurs -> (rows, the pairs: a set of ((i, a), (j, b)), i < j, level indices)"""
    rng = random.Random(seed)
    nf = len(factors)

    def row_of(idx):
        return dict(base, **{factors[i][0]: factors[i][1][a] for i, a in idx.items()})

    def fits(idx):                                        # (the exclusions are pairwise: a partial row is legal iff it is with the rest off)
        return legal(row_of(idx))

    need = {((i, a), (j, b)) for i in range(nf) for j in range(i + 1, nf) for a in range(len(factors[i][1]))
            for b in range(len(factors[j][1])) if fits({i: a, j: b})}
    every = set(need)
    rows = []
    while need:
        todo = sorted(need)
        best = None
        for _ in range(tries):
            (i, a), (j, b) = todo[rng.randrange(len(todo))]
            idx = {i: a, j: b}
            order = [k for k in range(nf) if k not in idx]
            rng.shuffle(order)
            for k in order:
                cands = []
                for v in range(len(factors[k][1])):
                    trial = dict(idx)
                    trial[k] = v
                    if not fits(trial):
                        continue
                    gain = sum(1 for m, u in idx.items() if (((k, v), (m, u)) if k < m else ((m, u), (k, v))) in need)
                    cands.append((gain, rng.random(), v))
                idx[k] = max(cands)[2]
            got = {((p, idx[p]), (q, idx[q])) for p in range(nf) for q in range(p + 1, nf)} & need
            if best is None or len(got) > len(best[0]):
                best = (got, idx)
        need -= best[0]
        rows.append(row_of(best[1]))
    return rows, every


def pairs_of(c, factors):
    """the pairs of level indices a call holds"""
    idx = [factors[i][1].index(c[factors[i][0]]) for i in range(len(factors))]
    return {((i, idx[i]), (j, idx[j])) for i in range(len(factors)) for j in range(i + 1, len(factors))}


@functools.lru_cache(maxsize=None)
def _pairs():
    return covering(FACTORS, OFF, seed=20261)


def pairs():
    """the rows of the resident entries: every legal pair of levels of FACTORS in at least one"""
    return [dict(r) for r in _pairs()[0]]


@functools.lru_cache(maxsize=None)
def _port_pairs():
    return covering(PORT_FACTORS, dict(OFF, entry="port"), seed=20262)


def port_pairs():
    """the rows of the port path: a covering array of its own over PORT_FACTORS"""
    return [dict(r) for r in _port_pairs()[0]]


def maximal():
    """the three largest legal sets, everything else on: name -> call"""
    on = dict(geom=FIT_TRUE, conformant=1, desc="repeat", stats=1, split=3)
    return {
        "sequences_schedule": call(seqs="batch", rate="sched", kind="nv12", pf=2, recon="i420", mux="ts", chunk=4, **on),
        "list_detector_schedule": call(layout="both", rate="sched", kind="rgbp", pf=3, recon="nv12", mux="ps", chunk=5, **on),
        "cap": call(rate="cap", kind="i420", pf=2, recon="nv12", mux="ts", chunk=4, **on),
    }


def setting(c, name):
    """the value of one of SETTINGS in a call ("size": the frame size set and its header mode, None with none set)"""
    if name == "size":
        return c["geom"] if c["geom"][2] else None
    return c[name]


def is_off(name, value):
    return value == setting(OFF, name)


def session_facts(calls):
    """what a session's order of calls does: (the fewest settings two consecutive calls differ in, the SETTINGS that are switched on,
    changed from one value to another and switched off between consecutive calls - the first call follows a handle with nothing set)"""
    fewest, on, changed, off = len(SETTINGS), set(), set(), set()
    prev = OFF
    for k, c in enumerate(calls):
        differ = 0
        for s in SETTINGS:
            a, b = setting(prev, s), setting(c, s)
            if a == b:
                continue
            differ += 1
            if is_off(s, a):
                on.add(s)
            elif is_off(s, b):
                off.add(s)
            else:
                changed.add(s)
        if k:
            fewest = min(fewest, differ)
        prev = c
    return fewest, on, changed, off


CHANGEABLE = {"size", "rate", "layout", "desc", "recon", "mux", "chunk", "split"}         # settings with two values besides "off"
ONOFF = set(SETTINGS) - {"split"}             # ("split_streams" is 1 or 3 in every row: never the default 2 again before the session's end)
SESSION_GEOMS = (PLAIN_GEOM,) * 3 + (FIT_TRUE, FIT_MODULE, FIT_TRUE) + (SMALL_GEOM,) * 3 + (PLAIN_GEOM,) * 3
SESSION_VLQ = (3, 2)


@functools.lru_cache(maxsize=None)
def _session(seed, vlq):
    rows = pairs()
    for attempt in range(4000):
        rng = random.Random(seed * 100003 + attempt)
        picked = rng.sample(rows, len(SESSION_GEOMS))
        calls = [dict(r, geom=g, vlq=vlq, entry=("block", "begin")[k % 2]) for k, (r, g) in enumerate(zip(picked, SESSION_GEOMS))]
        fewest, on, changed, off = session_facts(calls)
        if fewest >= 4 and on >= ONOFF and off >= ONOFF and changed >= CHANGEABLE:
            return tuple(calls)
    raise AssertionError("no order of rows found for the session")


SESSIONS = ((1, (3, 2)), (2, (3, 2)), (3, (1, 4)))          # (seed, the handle's levels) of the sessions tests/test_gpu_compose.py runs


def session(seed=1, vlq=SESSION_VLQ):
    """a dozen calls for ONE handle, rows of pairs() in a seeded order with the geometry going 96 x 64 -> 100 x 70 (a size set, coded
    112 x 80) -> 64 x 64 -> 96 x 64 and blocking calls and begin / end alternating: consecutive calls differ in at least four settings
    and every setting is switched on, changed and switched off at least once (session_facts)"""
    return [dict(c) for c in _session(seed, vlq)]


# ---- the material ----
@functools.lru_cache(maxsize=None)
def _base(w, h):
    W, H = F.padded(w, h)
    a = np.ascontiguousarray(M.synth.clip(W, H, N, CLIP_INDEX, scene_len=SCENE_LEN)[:, :, :h, :w])
    a.setflags(write=False)
    return a


def matrix_of(c):
    return "bt709" if c["kind"] == "rgbp" else "bt601"


@functools.lru_cache(maxsize=None)
def _source(w, h, kind):
    x = F.source(w, h, N, kind, seed=CLIP_INDEX, base=_base(w, h))
    x.setflags(write=False)
    return x


MATERIAL = {}                                 # name -> source frames [n, frame bytes] of other case modules (a call's "material")


def source(c):
    """the source frames of the call [n, frame bytes] in its kind, at its size: the clip of this module, or the call's "material" """
    if c.get("material"):
        return MATERIAL[c["material"]]
    return _source(c["geom"][0], c["geom"][1], c["kind"])


@functools.lru_cache(maxsize=None)
def _planes(w, h, kind, matrix):
    W, H = F.padded(w, h)
    p = np.ascontiguousarray(F.planes(_source(w, h, kind), w, h, kind, matrix).reshape(N, 3, H, W))
    p.setflags(write=False)
    return p


def planes(c):
    """the padded planar 4:4:4 frames the encoder is to code [n, 3, H, W]"""
    if c.get("material"):
        w, h, _ = c["geom"]
        x = MATERIAL[c["material"]]
        return F.planes(x.reshape(len(x), -1), w, h, c["kind"], matrix_of(c)).reshape((len(x), 3) + F.padded(w, h)[::-1])
    return _planes(c["geom"][0], c["geom"][1], c["kind"], matrix_of(c))


def nframes(c):
    return len(source(c))


# a factor's level is one of FACTORS' names, or the value itself: ("sched", levels), ("cap", B), ("starts", list or None, T), a tuple
# of lengths, a tuple of (field, value) of a description
def levels_of(c):
    r = c["rate"]
    if isinstance(r, tuple):
        return r[1] if r[0] == "sched" else r[2] if len(r) > 2 else None          # (("cap", B, levels): the cap starts from a schedule)
    return SCHEDULE if r == "sched" else None


def is_cap(c):
    return c["rate"] == "cap" or (isinstance(c["rate"], tuple) and c["rate"][0] == "cap")


def cap_of(c):
    return 0 if not is_cap(c) else cap_bytes(c) if c["rate"] == "cap" else c["rate"][1]


def starts_of(c):
    v = c["layout"]
    return v[1] if isinstance(v, tuple) else LIST if v in ("list", "both") else None


def cut_of(c):
    v = c["layout"]
    return v[2] if isinstance(v, tuple) else threshold(c) if v in ("cut", "both") else 0


def lengths_of(c):
    return None if not c["seqs"] else list(SEQS) if c["seqs"] == "batch" else list(c["seqs"])


def desc_of(c):
    """the description of the call as desc_cases' dict (the module's when none is set)"""
    if c["desc"] is None:
        return dict(D.MODULE)
    if isinstance(c["desc"], tuple):
        return D.desc(**dict(c["desc"]))
    return D.desc(repeat_headers=1 if c["desc"] == "repeat" else 0, **DESC)


def gop_alone(c, frames, q):
    """(the bytes of the one GOP of the oracle's stream of these frames encoded alone at level q, the dump of that encode)"""
    w, h, _ = c["geom"]
    W, H = F.padded(w, h)
    stream, dump = G.encoded(frames, W, H, c["pf"], q, VL=c["vlq"][0], conformant=bool(c["conformant"]))
    head, g = G.cut(stream)
    assert len(head) == G.SEQ_HEADER_BYTES and len(g) == 1 and g[0][:4] == G.GOP_CODE
    return g[0], dump


def threshold(c):
    """T of option "scene_cut" for this call, from D(n) of its padded frames: half way between the second and the third largest D(n),
    per macroblock - the two scene changes of the clip are flagged and nothing else (tests/test_compose_cases.py asserts it)"""
    p = planes(c)
    d = sorted(int(v) for v in SC.diffs(p)[1:])
    mbs = (p.shape[2] // 16) * (p.shape[3] // 16)
    return (d[-2] + d[-3]) // (2 * mbs)


def cap_bytes(c):
    """B of option "gop_bytes_max" for this call, from the oracle's sizes of its GOPs at the handle's Q_LEVEL: half way between the
    smallest and the largest - the largest GOP is coded again (where the handle is below level 4), the smallest is not"""
    p = planes(c)
    sizes = [len(gop_alone(c, p[s:s + L], c["vlq"][1])[0]) for s, L in SC.gops(len(p), c["pf"], None)]
    return (min(sizes) + max(sizes)) // 2


def stream_room(c):
    """bytes of the output buffer of a resident call"""
    xs, ys = M.fit_size(*c["geom"][:2])
    return nframes(c) * (3 * 256 * xs * ys + 128 + 34) + (1 << 16)


def mux_room(c):
    """bytes of the container buffer"""
    return M.mux_bound(c["mux"], stream_room(c), nframes(c)) + 64 * nframes(c) if c["mux"] else 0


def empty_reports():
    return dict(sequence_report=np.zeros(0, M.SEQUENCE_STAT_DTYPE), gop_report=np.zeros(0, M.GOP_STAT_DTYPE),
                scene_report=np.zeros(0, M.SCENE_STAT_DTYPE), picture_stats=np.zeros(0, M.PICTURE_STAT_DTYPE),
                mux_report=np.zeros(0, M.MUX_STAT_DTYPE))


REPORTS = ("sequence_report", "gop_report", "scene_report", "picture_stats", "mux_report")


# ---- the model ----
_expected = {}


def expected(c):
    """everything the library must hand back for the call: dict(stream, clips [the stream of every clip], offsets, marks [(offset,
    bytes, name) of every header and time code], the five reports, recon [N, frame bytes] or None, containers [bytes per clip] or None)"""
    assert legal(c), c
    key = tuple(sorted((k, v) for k, v in c.items() if k not in ("chunk", "split", "entry")))        # (no byte depends on these)
    if c.get("material"):
        return _compose(c)
    if key not in _expected:
        _expected[key] = _compose(c)
    return _expected[key]


def _compose(c):
    w, h, header = c["geom"]
    W, H = F.padded(w, h)
    pf, Qh = c["pf"], c["vlq"][1]
    p = planes(c)
    n = len(p)
    lengths = lengths_of(c) or [n]
    d = desc_of(c)
    hdr = D.seq_headers(*((w, h) if header == "true" else (W, H)), d)
    region = (w, h) if header else None
    starts, T = starts_of(c), cut_of(c)
    cuts = SC.cuts_of(p, T) if T else ()
    levels, B = levels_of(c), cap_of(c)
    out = empty_reports()
    clips, marks, stats, recon, gop_rec, at = [], [], [], [], [], 0
    for b, clip in enumerate(Q.split(p, lengths)):
        gs = SC.gops(len(clip), pf, starts, cuts)
        lv = G.per_gop(levels, len(gs)) if levels else [Qh] * len(gs)
        body = hdr
        marks.append((at, len(hdr), "sequence headers of clip %d" % b))
        for k, (s, L) in enumerate(gs):
            q, tries, over = lv[k], 1, 0
            if B:
                sizes = [[len(gop_alone(c, clip[s:s + L], qq)[0])] for qq in (1, 2, 3, 4)]
                (q,), (tries,), (over,) = G.cap_levels(sizes, [lv[k]], B)
            g, dump = gop_alone(c, clip[s:s + L], q)
            if k and d["repeat_headers"]:
                marks.append((at + len(body), len(hdr), "repeated headers of GOP %d of clip %d" % (k, b)))
                body += hdr
            marks.append((at + len(body) + 4, 4, "time code of GOP %d of clip %d" % (k, b)))
            body += g[:4] + D.time_code(s, d["frame_rate_code"]) + g[8:]
            if c["stats"]:
                r = S.records(dump, W, H, pf, region)
                r["frame"] += s                           # (frame numbers count from the clip's first frame)
                stats.append(r)
            recon.append(dump["recon"])
            gop_rec.append((k, s, L, q, len(g), tries, over))      # (bytes: the GOP without a repeated header in front)
        clips.append(G.finish(body))
        at += len(clips[-1])
    offsets = Q.lengths_offsets(clips)
    out.update(stream=b"".join(clips), clips=clips, offsets=offsets, marks=marks, lengths=lengths, recon=None, containers=None)
    if len(lengths) >= 2:
        out["sequence_report"] = Q.records(lengths, offsets, pf)
    if B:
        out["gop_report"] = np.array(gop_rec, M.GOP_STAT_DTYPE)
    if starts or T:
        out["scene_report"] = SC.records(n, pf, starts, cuts, SC.diffs(p) if T else None)
    if c["stats"]:
        out["picture_stats"] = np.concatenate(stats)
    if c["recon"]:
        out["recon"] = R.write_layout(np.concatenate(recon), W, H, c["recon"], region)
    if c["mux"]:
        out["containers"] = [X.cpu_mux(c["mux"], s) for s in clips]
        assert all(isinstance(v, bytes) for v in out["containers"]), "the CPU muxer refuses an expected stream"
        out["mux_report"] = mux_records(out, mux_room(c))
    return out


def mux_records(want, cap):
    """what m2v_mux_report must hand out for the expected containers in a buffer of cap bytes"""
    lay = X.layout([len(v) for v in want["containers"]], cap)
    r = np.zeros(len(lay), M.MUX_STAT_DTYPE)
    for b, (o, nb, st) in enumerate(lay):
        r[b] = (want["offsets"][b], len(want["clips"][b]), o, nb, want["lengths"][b] if st == 0 else 0, st)
    return r


def render(c, want=None):
    """what a call leaves behind that does everything right: dict(stream_buf (the whole output buffer, SENTINEL where nothing was
    written), nbytes, the five reports, recon_buf (FILL, GUARD bytes behind the frames) or None, mux_buf (SENTINEL) or None)"""
    want = want or expected(c)
    got = {k: want[k].copy() for k in REPORTS}
    buf = np.full(stream_room(c), SENTINEL, np.uint8)
    buf[:len(want["stream"])] = np.frombuffer(want["stream"], np.uint8)
    got.update(stream_buf=buf, nbytes=len(want["stream"]), recon_buf=None, mux_buf=None)
    if want["recon"] is not None:
        got["recon_buf"] = np.full(want["recon"].size + GUARD, FILL, np.uint8)
        got["recon_buf"][:want["recon"].size] = want["recon"].reshape(-1)
    if want["containers"] is not None:
        got["mux_buf"] = np.full(mux_room(c), SENTINEL, np.uint8)
        for r, v in zip(want["mux_report"], want["containers"]):
            got["mux_buf"][int(r["out_offset"]):int(r["out_offset"]) + len(v)] = np.frombuffer(v, np.uint8)
    return got


# ---- the comparison ----
class Mismatch(AssertionError):
    """what a call handed back is not what the model expects; item: the name of the first thing that differs"""

    def __init__(self, what, item, detail):
        AssertionError.__init__(self, "%s: %s: %s" % (what, item, detail))
        self.item = item


def _mark(want, at):
    for o, n, name in want["marks"]:
        if o <= at < o + n:
            return " (%s)" % name
    b = max(k for k, o in enumerate(want["offsets"][:-1]) if o <= at) if at < want["offsets"][-1] else len(want["clips"]) - 1
    return " (clip %d, byte %d of it)" % (b, at - want["offsets"][b])


def check(got, want, what=""):
    """everything a call handed back (as render() lays it out) against expected(call), byte for byte and integer for integer; raises
    Mismatch naming the first item that differs"""
    es = want["stream"]
    if got["nbytes"] != len(es):
        raise Mismatch(what, "stream length", "%d bytes, expected %d" % (got["nbytes"], len(es)))
    buf = np.asarray(got["stream_buf"])
    bad = np.flatnonzero(buf[:len(es)] != np.frombuffer(es, np.uint8))
    if bad.size:
        raise Mismatch(what, "stream", "%d bytes differ, the first at %d%s" % (bad.size, bad[0], _mark(want, int(bad[0]))))
    bad = np.flatnonzero(buf[len(es):] != SENTINEL)
    if bad.size:
        raise Mismatch(what, "stream sentinel", "byte %d behind the stream's %d changed" % (bad[0], len(es)))
    for name in REPORTS:
        g, w = got[name], want[name]
        if g.dtype != w.dtype or len(g) != len(w):
            raise Mismatch(what, name, "%d records, expected %d" % (len(g), len(w)))
        for field in w.dtype.names:
            if not np.array_equal(g[field], w[field]):
                k = int(np.flatnonzero((g[field] != w[field]).reshape(len(w), -1).any(axis=1))[0])
                raise Mismatch(what, "%s.%s" % (name, field), "record %d: %r, expected %r" % (k, g[field][k].tolist(), w[field][k].tolist()))
    if (got["recon_buf"] is None) != (want["recon"] is None):
        raise Mismatch(what, "recon", "a buffer where none is expected, or none where one is")
    if want["recon"] is not None:
        rb, fb = np.asarray(got["recon_buf"]), want["recon"].shape[1]
        bad = np.flatnonzero(rb[:want["recon"].size] != want["recon"].reshape(-1))
        if bad.size:
            raise Mismatch(what, "recon", "%d bytes differ, the first is byte %d of frame %d" % (bad.size, bad[0] % fb, bad[0] // fb))
        bad = np.flatnonzero(rb[want["recon"].size:] != FILL)
        if bad.size:
            raise Mismatch(what, "recon guard", "byte %d behind the last frame changed" % bad[0])
    if (got["mux_buf"] is None) != (want["containers"] is None):
        raise Mismatch(what, "container", "a buffer where none is expected, or none where one is")
    if want["containers"] is not None:
        mb = np.asarray(got["mux_buf"])
        touched = np.zeros(mb.size, bool)
        for b, (r, v) in enumerate(zip(want["mux_report"], want["containers"])):
            o = int(r["out_offset"])
            bad = np.flatnonzero(mb[o:o + len(v)] != np.frombuffer(v, np.uint8))
            if bad.size:
                raise Mismatch(what, "container %d" % b, "%d bytes differ, the first at %d of %d" % (bad.size, bad[0], len(v)))
            touched[o:o + len(v)] = True
        bad = np.flatnonzero(mb[~touched] != SENTINEL)
        if bad.size:
            raise Mismatch(what, "container sentinel", "a byte outside the reported ranges changed (%d of them)" % bad.size)
