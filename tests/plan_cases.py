"""The main-syntax decode plans (k_dm_plan, k_db_plan, k_di_plan, k_dx_plan, k_dt_plan and, per stream of a batch, k_dsm_plan) on streams
longer than a lane's range: the streams, a model of the partition, and what the streams must reach - shared by tests/test_plan_cases.py
(CPU) and tests/test_gpu_decode_plan.py.  Every plan cuts the event list into 256 ranges of per = ceil(nev / 256) events; each lane
summarises its own range, lane 0 makes the exclusive sums, and each lane fills in its pictures from what the lanes in front carried.
The streams of the other suites have per = 1 (one of them 2); these have per 1 .. 13, so that a range holds several pictures.

The definition is the expectation: decoder.decode(stream, quirks=False, syntax="main", b_pictures=, interlaced=, extended=, mb_tools=) -
its frames, or the offset its Refused names.  The host builds (tools/dec_*_host.hpp) plan serially; tests/test_plan_cases.py holds them
to the definition on every stream.  Nothing here looks at what the device computes.

Content: tiny pictures (16 x 16, 16 x 32 with progressive_sequence 0, 48 x 16) that are nearly flat - an I picture says its level, a P
picture adds a residual that is never zero, B pictures come forward-only, backward-only and bidirectional in turn - so a plan that
picks the wrong reference, matrix or display slot changes bytes; content_faults() states the rule.  Streams are written by
ext_writer.stream (main_writer's, bpic_writer's and ilace_writer's pictures) and mbt_writer.stream; the one new writer piece is
users(k).

An options tuple is (b_pictures, interlaced, extended, mb_tools)."""
import functools

import numpy as np

import bpic_cases as BC
import dec_cases as D
import ext_cases as X
import ext_writer as XW
import ilace_cases as IC
import main_cases as C
import mbt_cases as T
import mbt_writer as TW

M = D.M
Refused = M.decoder.Refused
THREADS = 256                                                       # kDecThreads
M_, B_, I_, BI, XO, XB, XBI, TO = (0, 0, 0, 0), (1, 0, 0, 0), (0, 1, 0, 0), (1, 1, 0, 0), (0, 0, 1, 0), (1, 0, 1, 0), (1, 1, 1, 0), (1, 0, 1, 1)
PLAN_OF = {M_: "k_dm_plan", B_: "k_db_plan", I_: "k_di_plan", BI: "k_di_plan", XO: "k_dx_plan", XB: "k_dx_plan", XBI: "k_dx_plan", TO: "k_dt_plan",
           (1, 1, 1, 1): "k_dt_plan"}


def spec(stream, opt):
    """-> (Decoded, None) or (None, the offset of the unit the definition refuses)"""
    b, i, x, t = (bool(v) for v in opt)
    try:
        return M.decoder.decode(bytes(stream), quirks=False, syntax="main", b_pictures=b, interlaced=i, extended=x, mb_tools=t), None
    except Refused as e:
        return None, e.offset


_specs = {}


def spec_cached(stream, opt):
    key = (bytes(stream), tuple(bool(v) for v in opt))
    if key not in _specs:
        _specs[key] = spec(*key)
    return _specs[key]


def host_decode(stream, opt, layout="i420"):
    """the g++ build of the option's functions with its serial plan -> (frames or None, the record)"""
    b, i, x, t = (bool(v) for v in opt)
    if t:
        return T.host_decode(stream, b, i, layout)
    if x:
        return X.host_decode(stream, b, i, layout)
    if i:
        return IC.host_decode(stream, b, layout)
    return BC.host_decode(stream, layout) if b else C.host_decode(stream, layout)


record_of = C.record_of


# ---- the partition: the one line all six kernels share ----
def per_of(nev):
    return (nev + THREADS - 1) // THREADS


def ranges(nev):
    """lane t holds the events [a, b)"""
    per = per_of(nev)
    return [(min(nev, t * per), min(nev, t * per + per)) for t in range(THREADS)]


def first_guess(nbytes):
    """the event list's first size in m2v_decode_device"""
    return max(1024, nbytes // 16 + 64)


# ---- the new writer piece ----
def users(k, tag=0):
    """k short user_data units, for wherever a transparent unit may stand (behind a sequence's extensions, a GOP header, a picture
    coding extension)"""
    return [("user", b"\x00\x00\x01\xb2" + bytes([0x41 + (tag + j) % 26])) for j in range(k)]


# ---- content ----
def _own(m):
    m = list(m)
    m[0] = 16                                                       # (a P picture's flat residual keeps its size under every matrix)
    return m


MATS = tuple(_own(m) for m in (C.MATRIX_A, C.MATRIX_B, [12 + (7 * i) % 45 for i in range(64)], [20 + (11 * i) % 33 for i in range(64)]))
assert len({m[1] for m in MATS} | {16}) == 5                        # raster 1, where every picture has a coefficient: all differ, and from both defaults
I_AC = ((0, 6), (0, -5))                                            # an intra block's coefficients at scan positions 1 and 2
P_AC = ((0, 3), (0, -2))                                            # a residual block's, behind its coefficient at position 0
B_LEVELS = (2, -2, 3, -3, 1, -1)


def intra_pic(v, mbw, mbh, **kw):
    """every sample about v (intra_dc_precision 0), block 0 of every macroblock with I_AC"""
    mb = lambda col: dict(kind="intra", blocks=[dict(dc=(v - 128) if col == 0 and b in (0, 4, 5) else 0, coefs=[(r, l, False) for r, l in I_AC] if b == 0 else [])
                                                for b in range(6)])
    return dict(type=1, prec=0, slices=[dict(q=4, mbs=[mb(col) for col in range(mbw)]) for _ in range(mbh)], **kw)


def _residual(level, ac):
    return [dict(coefs=[(0, level, False)] + ([(r, l, False) for r, l in ac] if b == 0 else [])) for b in range(6)]


def p_pic(level, mbw, mbh, flip=False, **kw):
    """the reference plus a flat residual of `level` (never 0) in all six blocks; flip: P_AC with the other signs, so that a run of P
    pictures does not pile them up"""
    assert level
    ac = tuple((r, -l if flip else l) for r, l in P_AC)
    return dict(type=2, slices=[dict(q=4, mbs=[dict(kind="coded", mv=(0, 0), cbp=63, blocks=_residual(level, ac)) for _ in range(mbw)]) for _ in range(mbh)], **kw)


def b_pic(mode, level, run, mbw, mbh, **kw):
    """mode 0 forward, 1 backward, 2 both; level 0: no residual; a coefficient `run` positions behind the first tells B pictures apart"""
    fwd, bwd = ((0, 0) if mode != 1 else None), ((0, 0) if mode != 0 else None)
    mb = lambda: BC.pred(fwd, bwd) if not level else dict(BC.pred(fwd, bwd), cbp=63, blocks=_residual(level, ((0, 4), (run, 1))))
    return dict(type=3, slices=[dict(q=3, mbs=[mb() for _ in range(mbw)]) for _ in range(mbh)], **kw)


def refs_of(types):
    """per coded picture (forward, backward) as coded indices, None where it has none"""
    out, a1, a2 = [], None, None
    for p, t in enumerate(types):
        out.append((a1, None) if t == 2 else (a2, a1) if t == 3 else (None, None))
        if t != 3:
            a1, a2 = p, a1
    return out


def display_of(types):
    """the display index of every coded picture: a B picture goes out when decoded, an anchor when the next one arrives"""
    out, shown, held = [0] * len(types), 0, None
    for p, t in enumerate(types):
        if t != 3 and held is not None:
            out[held], shown = shown, shown + 1
        if t == 3:
            out[p], shown = shown, shown + 1
        else:
            held = p
    if held is not None:
        out[held] = shown
    return out


def pictures(letters, mbw=1, mbh=1, seed=1, gops=(), seqs=(), loads=None, all_residual=False, closed=()):
    """letters in coded order ("IPBBPBB...") -> the writer's pictures.  gops / seqs: the coded indices with a GOP header / a repeated
    sequence header in front (0 has both); loads: coded index -> (intra matrix or None, non-intra matrix or None), a
    quant_matrix_extension behind that picture's coding extension.  Levels are chosen so that the last four anchors differ by 2 at
    least and everything stays between 50 and 200"""
    rng = np.random.RandomState(seed)
    out, est, nb = [], [], 0
    for k, c in enumerate(letters):
        kw = dict(seq=k == 0 or k in seqs, gop=k == 0 or k in gops)
        if kw["gop"] and letters[k + 1:k + 2] == "B" and k not in closed:
            kw["open_gop"] = True
        if loads and k in loads:
            kw["extras"] = [XW.quant_ext(intra=loads[k][0], non_intra=loads[k][1])]
        if c == "I":
            for _ in range(100):
                v = int(rng.randint(70, 181))
                if all(abs(v - e) >= 6 for e in est[-3:]):
                    break
            est.append(v)
            out.append(intra_pic(v, mbw, mbh, **kw))
        elif c == "P":
            step = lambda l: l + (l > 0) - (l < 0)                  # about what a level adds to every sample
            ok = [l for l in (1, -1, 2, -2, 3, -3, 4, -4, 5, -5, 6, -6) if 50 <= est[-1] + step(l) <= 200 and all(abs(est[-1] + step(l) - e) >= 2 for e in est[-3:])]
            if est[-1] > 160 or est[-1] < 90:                        # (back towards the middle where that is possible)
                ok = [l for l in ok if (l < 0) == (est[-1] > 125)] or ok
            assert ok, (k, est[-4:])
            l = ok[int(rng.randint(len(ok)))]
            est.append(est[-1] + step(l))
            out.append(p_pic(l, mbw, mbh, flip=bool(len(est) & 1), **kw))
        else:
            mode = nb % 3
            level = B_LEVELS[nb % 6] if (mode != 2 or all_residual or nb % 2) else 0
            out.append(b_pic(mode, level, 1 + nb % 5, mbw, mbh, **kw))
            nb += 1
    return out


def content_faults(frames, types):
    """the content rule on a stream's decoded frames (display order, [n, bytes]) -> the list of what breaks it"""
    bad = []
    f = np.asarray(frames)
    if f.min() == 0 or f.max() == 255:
        bad.append("a sample at 0 or 255")
    for d in range(len(f)):
        for e in range(d + 1, min(len(f), d + 5)):
            if np.array_equal(f[d], f[e]):
                bad.append("display %d and %d are equal" % (d, e))
    disp = display_of(types)
    anchors = [disp[p] for p, t in enumerate(types) if t != 3]
    for k in range(len(anchors)):
        for j in range(k + 1, min(len(anchors), k + 4)):
            a, b = f[anchors[k]], f[anchors[j]]
            if np.array_equal(a, b) or int(a.sum()) == int(b.sum()):
                bad.append("anchors %d and %d: equal frames or equal means" % (k, j))
    return bad


# ---- what a stream holds, from the start codes alone ----
TRANSPARENT, SIGNIFICANT = 0, 1
CROSSINGS = ("anchors_0", "anchors_1", "anchors_2", "anchors_3_or_more", "one_anchor_behind_none", "b_anchors_in_two_earlier_ranges",
             "b_anchors_in_one_earlier_range", "b_anchor_in_own_range", "p_reference_first_of_range", "p_reference_two_ranges_back", "i_last_of_range",
             "i_first_of_range", "cut_header_extension", "cut_extension_slice", "cut_slice_slice", "cut_gop_picture", "next_anchor_two_ranges_behind",
             "last_anchor", "load_used_two_ranges_behind", "sequence_then_load", "load_then_sequence", "transparent_only", "empty_lanes", "event_list_regrown",
             "more_than_256_pictures")


def events_of(stream):
    """[(offset, kind)]: kind "seq" "seq_ext" "display" "gop" "pic1" "pic2" "pic3" "pic_ext" "quant" "slice" "end" "skip" "other" """
    out = []
    for pos, code in M.decoder.start_codes(bytes(stream)):
        if code == 0x00:
            kind = "pic%d" % ((stream[pos + 5] >> 3) & 7) if pos + 5 < len(stream) else "other"
        elif code <= 0xAF:
            kind = "slice"
        elif code == 0xB5:
            kind = {1: "seq_ext", 2: "display", 8: "pic_ext", 3: "quant", 4: "skip", 7: "skip"}.get(stream[pos + 4] >> 4 if pos + 4 < len(stream) else 0, "other")
        else:
            kind = {0xB3: "seq", 0xB8: "gop", 0xB7: "end", 0xB2: "skip"}.get(code, "other")
        out.append((pos, kind))
    return out


def layout_of(stream):
    """the stream's pictures and their lanes: dict(nev, per, lane(i), kinds, pictures=[dict(ev, type, ext, slices, quant, lane)])"""
    ev = events_of(stream)
    kinds = [k for _, k in ev]
    per = max(1, per_of(len(ev)))
    pics = []
    for i, k in enumerate(kinds):
        if k in ("pic1", "pic2", "pic3"):
            pics.append(dict(ev=i, type=int(k[3]), ext=None, slices=[], quant=None, lane=i // per))
        elif pics and k == "pic_ext" and pics[-1]["ext"] is None:
            pics[-1]["ext"] = i
        elif pics and k == "slice":
            pics[-1]["slices"].append(i)
        elif pics and k == "quant":
            pics[-1]["quant"] = i
    return dict(nev=len(ev), per=per, kinds=kinds, pictures=pics, offsets=[p for p, _ in ev])


def reached(stream):
    """the names of CROSSINGS that the stream holds, in CROSSINGS' order"""
    L = layout_of(stream)
    nev, per, kinds, pics = L["nev"], L["per"], L["kinds"], L["pictures"]
    lane = lambda i: i // per
    lanes = (nev + per - 1) // per                                   # the lanes that hold an event
    types = [p["type"] for p in pics]
    refs = refs_of(types)
    got = set()
    anchors_in = [0] * lanes
    first_pic, last_pic = {}, {}
    for n, p in enumerate(pics):
        anchors_in[p["lane"]] += p["type"] != 3
        first_pic.setdefault(p["lane"], n)
        last_pic[p["lane"]] = n
    for t in range(lanes):
        got.add(("anchors_0", "anchors_1", "anchors_2", "anchors_3_or_more")[min(3, anchors_in[t])])
        if t and anchors_in[t] == 1 and anchors_in[t - 1] == 0:
            got.add("one_anchor_behind_none")
        if all(k == "skip" for k in kinds[t * per:t * per + per]):
            got.add("transparent_only")
    anchors = [n for n, p in enumerate(pics) if p["type"] != 3]
    for n, p in enumerate(pics):
        f, b = refs[n]
        if p["type"] == 3 and f is not None and b is not None:
            lf, lb = pics[f]["lane"], pics[b]["lane"]
            if lf < p["lane"] and lb < p["lane"]:
                got.add("b_anchors_in_two_earlier_ranges" if lf != lb else "b_anchors_in_one_earlier_range")
            if lb == p["lane"]:
                got.add("b_anchor_in_own_range")
        if p["type"] == 2 and f is not None:
            if pics[f]["lane"] == p["lane"] and first_pic[p["lane"]] == f:
                got.add("p_reference_first_of_range")
            if pics[f]["lane"] <= p["lane"] - 2:
                got.add("p_reference_two_ranges_back")
        if p["type"] == 1:
            if last_pic[p["lane"]] == n:
                got.add("i_last_of_range")
            if first_pic[p["lane"]] == n:
                got.add("i_first_of_range")
        if p["ext"] is not None and lane(p["ext"]) != p["lane"]:
            got.add("cut_header_extension")
        if p["ext"] is not None and p["slices"] and lane(p["slices"][0]) != lane(p["ext"]):
            got.add("cut_extension_slice")
        if any(lane(a) != lane(b) for a, b in zip(p["slices"], p["slices"][1:])):
            got.add("cut_slice_slice")
        back = p["ev"] - 1
        while back >= 0 and kinds[back] == "skip":
            back -= 1
        if back >= 0 and kinds[back] == "gop" and lane(back) != p["lane"]:
            got.add("cut_gop_picture")
    for a, b in zip(anchors, anchors[1:]):
        if pics[b]["lane"] >= pics[a]["lane"] + 2:
            got.add("next_anchor_two_ranges_behind")
    if anchors:
        got.add("last_anchor")
    # the matrices: a load, the pictures behind it until the next load of either matrix or a sequence header
    src = None
    for i, k in enumerate(kinds):
        if k == "seq" and i:
            src = None
            t = lane(i)
            if "quant" in kinds[i + 1:t * per + per]:
                got.add("sequence_then_load")
            if "quant" in kinds[t * per:i]:
                got.add("load_then_sequence")
        elif k == "quant":
            src = i
        elif k in ("pic1", "pic2", "pic3") and src is not None and lane(i) >= lane(src) + 2:
            got.add("load_used_two_ranges_behind")
    if lanes < THREADS:
        got.add("empty_lanes")
    if nev > first_guess(len(stream)):
        got.add("event_list_regrown")
    if len(pics) > 256:
        got.add("more_than_256_pictures")
    return [c for c in CROSSINGS if c in got]


# ---- the streams: name -> (stream, log, options, letters in coded order) ----
def _xw(w, h, pics, seq=None, rows=None):
    return XW.stream(w, h, pics, seq=seq, rows=rows)


EDGES = (255, 256, 257, 511, 512, 513, 767, 769)


def edge(n):
    """I B B P (coded I P B B) of 16 x 16, padded with user_data to exactly n start codes: behind the sequence's extensions and behind
    every coding extension"""
    letters = "IPBB"
    pad = n - 17
    share = [pad // 5 + (pad % 5 if k == 0 else 0) for k in range(5)]
    pics = pictures(letters, seed=n)
    for k, p in enumerate(pics):
        p["extras"] = users(share[k + 1], k)
    s, L = _xw(16, 16, pics, seq=dict(extras_behind=users(share[0], 7)))
    assert len(M.decoder.start_codes(s)) == n
    return s, L, B_, letters


def ipbb_letters(n):
    """I B B P B B P ... in display order with a new I picture every 12 pictures, in coded order: I B B P B B P B B P B B a GOP (the
    first one, which has no anchor in front of it, I P B B P B B P B B P P), n pictures"""
    return ("IPBBPBBPBBPP" + "IBBPBBPBBPBB" * (n // 12))[:n]


SHIFT_SEQ = dict(intra_matrix=MATS[0], non_intra_matrix=MATS[1])


def shift(k, interlaced=False, change=None):
    """about 1 800 events; k user_data units behind every sequence header's extensions.  A GOP header at every I picture (every 12
    pictures), a repeated sequence header with the matrices at every fourth GOP.  interlaced: progressive_sequence 0, coded 16 x 32,
    two slices.  change(pictures): a twin"""
    n = 400 if interlaced else 540
    letters = ipbb_letters(n)
    gops = {p for p in range(n) if letters[p] == "I"}
    pics = pictures(letters, 1, 2 if interlaced else 1, seed=11, gops=gops, seqs={p for p in gops if p % 48 == 0})
    if change:
        change(pics)
    seq = dict(SHIFT_SEQ, extras_behind=users(k, 3))
    if interlaced:
        seq["progressive"] = 0
    s, L = _xw(16, 32 if interlaced else 16, pics, seq=seq, rows=2 if interlaced else None)
    return s, L, BI if interlaced else B_, letters


SHIFT_PER = 7


def seeded_letters(n, seed, b=True):
    """runs of I, P, B B, B B B, an I straight behind an I, P P P P without B -> (letters, GOP headers, repeated sequence headers, the
    GOP headers that say closed_gop)"""
    rng = np.random.RandomState(seed)
    out, gops, seqs, closed = ["I", "P"], set(), set(), set()
    while len(out) < n:
        r = int(rng.randint(12))
        if r == 0:
            gops.add(len(out))
            if rng.randint(3) == 0:
                seqs.add(len(out))
            if rng.randint(2):
                closed.add(len(out))
            out += ["I"] + (["B", "B"] if b and rng.randint(2) else [])
        elif r == 1:
            gops.add(len(out))
            out += ["I", "I"]
        elif r == 2:
            out += ["P"] * 4
        elif r == 3:
            out += ["I"]                                             # an I picture without a GOP header
        elif not b:
            out += ["P"]
        else:
            out += ["P"] + ["B"] * (2, 2, 2, 3, 3, 1, 0, 2)[int(rng.randint(8))]
    return "".join(out[:n]), {g for g in gops if g < n}, {g for g in seqs if g < n}, closed


def long_b():
    letters, gops, seqs, closed = seeded_letters(1000, 21)
    s, L = _xw(16, 16, pictures(letters, seed=22, gops=gops, seqs=seqs, closed=closed))
    return s, L, B_, letters


def long_m():
    letters, gops, seqs, closed = seeded_letters(470, 23, b=False)
    s, L = _xw(16, 16, pictures(letters, seed=24, gops=gops, seqs=seqs))
    return s, L, M_, letters


def x_loads(letters, seqs, seed):
    """quant_matrix_extension at about every ninth picture: each matrix alone and both together, in turn; and at the picture in front
    of every repeated sequence header and at the one behind it, so that a header can share a range with a load on either side (X_SEQS
    is chosen so that the first one does); a load never repeats the matrix in force.  -> coded index -> (intra, non-intra)"""
    rng = np.random.RandomState(seed)
    loads, n, cur = {}, 0, [2, 3]                                   # (X_SEQ's matrices are in force)
    at = set(range(4, len(letters), 9)) | {s - 1 for s in seqs} | set(seqs)
    for p in range(len(letters)):
        if p in seqs:
            cur = [2, 3]
        if p not in at:
            continue
        new = [[j for j in range(4) if j != cur[m]][int(rng.randint(3))] for m in range(2)]      # never the one in force
        kind = n % 3
        loads[p] = (MATS[new[0]] if kind != 1 else None, MATS[new[1]] if kind != 0 else None)
        cur = [new[m] if loads[p][m] is not None else cur[m] for m in range(2)]
        n += 1
    return loads


def x_cuts(pics, seed, mbw=3):
    """one to three slices a row, cut at seeded columns"""
    rng = np.random.RandomState(seed)
    out = []
    for p in pics:
        cut = sorted(set(int(c) for c in rng.randint(1, mbw, size=int(rng.randint(3)))))
        out.append(dict(p, cuts=[cut for _ in p["slices"]]))
    return out


X_SEQ = dict(intra_matrix=MATS[2], non_intra_matrix=MATS[3])


X_SEQS = (167, 390)                                                   # two I pictures: a repeated sequence header (no GOP header) in front


def x_pictures(change=None, seqs=None):
    letters, gops, _, closed = seeded_letters(520, 25)
    seqs = set(X_SEQS if seqs is None else seqs)
    assert all(letters[p] == "I" for p in seqs)
    gops -= seqs
    loads = x_loads(letters, seqs, 26)
    if change:
        loads, seqs = change(dict(loads), set(seqs))
    pics = x_cuts(pictures(letters, 3, 1, seed=27, gops=gops, seqs=seqs, loads=loads, all_residual=True, closed=closed), 28)
    return pics, letters, loads, seqs


def long_x(change=None):
    """48 x 16 (three macroblocks, so that a row has up to three slices) under decode_extended"""
    pics, letters, loads, seqs = x_pictures(change)
    s, L = _xw(48, 16, pics, seq=X_SEQ)
    return s, L, XB, letters


def long_t():
    """long_x's pictures with intra_vlc_format 1 and concealment vectors, under decode_mb_tools"""
    pics, letters, loads, seqs = x_pictures()
    for k, p in enumerate(pics):
        for sl in p["slices"]:
            for col, m in enumerate(sl["mbs"]):
                if m["kind"] == "intra":
                    m["cmv"] = ((k % 5) - 2, (col + k) % 3 - 1)
    s, L = TW.stream(48, 16, T.with_flags(pics, ivf=1, cmv=1), seq=X_SEQ)
    return s, L, TO, letters


@functools.lru_cache(maxsize=None)
def cases():
    out = {}
    for n in EDGES:
        out["edge_%d" % n] = edge(n)
    for k in range(SHIFT_PER):
        out["shift_%d" % k] = shift(k)
        out["shift_%d_interlaced" % k] = shift(k, True)
    out["long_b"] = long_b()
    out["long_x"] = long_x()
    out["long_t"] = long_t()
    out["long_m"] = long_m()
    return out


def later_options(opt):
    """the option sets of the later plans that accept a stream which needs opt (each plan once)"""
    order = (M_, B_, BI, XBI, (1, 1, 1, 1))
    return [o for o in order if all(o[k] >= opt[k] for k in range(4)) and o != tuple(opt)]


# ---- sensitivity: twins in which one carried quantity's source differs ----
def closure(types, own):
    """the coded pictures that change when those of `own` do: they, and whatever predicts from a changed picture (pictures() gives B
    picture number nb the directions nb % 3: forward, backward, both)"""
    refs, out, nb = refs_of(types), set(own), 0
    for p in range(len(types)):
        used = refs[p]
        if types[p] == 3:
            used, nb = (refs[p][:1], refs[p][1:], refs[p])[nb % 3], nb + 1
        if any(r is not None and r in out for r in used):
            out.add(p)
    return out


def mats_in_force(letters, loads, seqs):
    """per coded picture the (intra, non-intra) sources: the coded index of the picture whose extension loaded it, None: the sequence's"""
    out, cur = [], [None, None]
    for p in range(len(letters)):
        if p in seqs:
            cur = [None, None]
        if p in loads:
            cur = [p if loads[p][m] is not None else cur[m] for m in range(2)]
        out.append(tuple(cur))
    return out


def matrix_twin(kind):
    """long_x with one load ("load") or one repeated sequence header ("reset") removed -> (stream, twin, the coded pictures that must
    change, the event of the source, letters)"""
    pics, letters, loads, seqs = x_pictures()
    if kind == "load":
        gone = sorted(loads)[len(loads) // 2]
        change = lambda l, s: ({k: v for k, v in l.items() if k != gone}, s)
    else:
        gone = sorted(seqs)[0]
        change = lambda l, s: (l, s - {gone})
    loads2, seqs2 = change(dict(loads), set(seqs))
    before, after = mats_in_force(letters, loads, seqs), mats_in_force(letters, loads2, seqs2)

    def weights(p, src, m):
        return tuple((X_SEQ["intra_matrix"], X_SEQ["non_intra_matrix"])[m] if src is None else loads[src][m])        # (None: the sequence's)
    own = set()
    for p, c in enumerate(letters):
        m = 0 if c == "I" else 1                                     # an I picture's blocks are intra, every other block is a residual
        if weights(p, before[p][m], m) != weights(p, after[p][m], m):
            own.add(p)
    s = long_x()[0]
    twin = long_x(change)[0]
    return s, twin, closure([" IPB".index(c) for c in letters], own), gone, letters


def shift_twin(kind):
    """shift_0 with one anchor's level changed ("anchor") or two adjacent B pictures' contents exchanged ("swap") -> (stream, twin, the
    display indices that must change, the coded index of the source, letters)"""
    s, L, opt, letters = shift(0)
    types = [" IPB".index(c) for c in letters]
    disp = display_of(types)
    lay = layout_of(s)
    if kind == "anchor":
        # a P picture that is the last picture of its range: what hangs on it lies in later ranges
        src = next(p for p in range(100, len(types)) if types[p] == 2 and types[p + 1] == 3 and lay["pictures"][p + 1]["lane"] > lay["pictures"][p]["lane"])

        def change(pics):
            lv = pics[src]["slices"][0]["mbs"][0]["blocks"][0]["coefs"][0][1]
            pics[src] = p_pic(lv + 3 if lv > 0 else lv - 3, 1, 1, **{k: v for k, v in pics[src].items() if k in ("seq", "gop", "open_gop")})
        want = {disp[p] for p in closure(types, {src})}
    else:
        src = next(p for p in range(100, len(types) - 1) if types[p] == 3 and types[p + 1] == 3 and lay["pictures"][p + 1]["lane"] > lay["pictures"][p]["lane"])

        def change(pics):
            keep = lambda q: {k: v for k, v in q.items() if k in ("seq", "gop", "open_gop")}
            a, b = pics[src], pics[src + 1]
            pics[src], pics[src + 1] = dict({k: v for k, v in b.items() if k not in ("seq", "gop", "open_gop")}, **keep(a)), \
                dict({k: v for k, v in a.items() if k not in ("seq", "gop", "open_gop")}, **keep(b))
        want = {disp[src], disp[src + 1]}
    twin = shift(0, change=change)[0]
    return s, twin, want, src, letters


# ---- refusals stated by hand: name -> (stream, options, the offset, or None where the stream is accepted) ----
def _unit(L, kind, nth):
    return [a for k, a in L["units"] if k == kind][nth]


def _drop(s, L, at):
    """the stream without the unit at offset `at`"""
    offs = [a for _, a in L["units"]] + [len(s)]
    return s[:at] + s[offs[offs.index(at) + 1]:]


@functools.lru_cache(maxsize=None)
def refusals():
    out = {}
    # I, user_data for several ranges, B: the B picture has one anchor in front of it
    pics = pictures("IPB", seed=31)
    ib = [dict(pics[0], extras=users(600)), pics[2]]
    s, L = _xw(16, 16, ib)
    out["i_far_b"] = (s, B_, _unit(L, "picture", 1))
    ipb = [dict(pics[0], extras=users(600)), dict(pics[1], extras=users(300, 5)), pics[2]]
    s, L = _xw(16, 16, ipb)
    out["i_far_p_far_b"] = (s, B_, None)
    # two faults about 1 000 events apart in long_b (a slice whose code is 2 in a picture of one row): the earlier one is named
    s, L, opt, letters = long_b()
    slices = [a for k, a in L["units"] if k == "slice"]
    lo, hi = slices[400], slices[730]
    one = bytearray(s); one[hi + 3] = 2; one[lo + 3] = 2
    two = bytearray(s); two[lo + 3] = 2; two[hi + 3] = 2
    assert one == two
    out["two_faults"] = (bytes(one), B_, lo)
    out["later_fault_alone"] = (s[:hi + 3] + b"\x02" + s[hi + 4:], B_, hi)
    # the B option off: named at the first B picture
    first_b = [a for (k, a), t in zip([u for u in L["units"] if u[0] == "picture"], letters) if t == "B"][0]
    out["b_option_off"] = (s, M_, first_b)
    # a picture header at a range's last event whose coding extension is missing: the slice behind it is named
    s, L, opt, letters = shift(0)
    lay = layout_of(s)
    p = next(q for q in lay["pictures"][60:] if q["ext"] // lay["per"] != q["lane"])
    ext = lay["offsets"][p["ext"]]
    cut = _drop(s, L, ext)
    assert per_of(lay["nev"] - 1) == lay["per"]
    out["extension_missing_at_range_end"] = (cut, B_, ext)          # (the slice moved up to where the extension stood)
    # a discontinuous slice in long_x far behind the first chunk: the middle one of three slices of a row is gone
    s, L, opt, letters = long_x()
    lay = layout_of(s)
    p = next(q for q in lay["pictures"][300:] if len(q["slices"]) == 3)
    mid = lay["offsets"][p["slices"][1]]
    out["gap_behind_first_chunk"] = (_drop(s, L, mid), XB, mid)     # (the slice behind the gap stands there now)
    return out


# ---- altered streams ----
@functools.lru_cache(maxsize=None)
def altered_base():
    """about 600 events (per 3), about 150 pictures of 16 x 16"""
    letters = ipbb_letters(190)
    gops = {p for p in range(len(letters)) if letters[p] == "I"}
    s, L = _xw(16, 16, pictures(letters, seed=41, gops=gops, seqs={48, 144}))
    return s, L, letters


@functools.lru_cache(maxsize=None)
def altered(n=120):
    """[(name, stream)]: seeded bit flips in a start code's value byte and the four bytes behind it, anywhere in the stream; cuts and
    insertions (decoded with "decode_b_pictures" on)"""
    s, L, letters = altered_base()
    rng = np.random.RandomState(42)
    offs = [a for _, a in L["units"]]
    out = []
    for k in range(n):
        at = offs[int(rng.randint(len(offs)))]
        if k % 4 < 2:
            bit = 8 * (at + 3) + int(rng.randint(40))
            if bit >= 8 * len(s):
                bit = 8 * (at + 3) + int(rng.randint(8))
            out.append(("flip%d" % bit, D.flip(s, bit)))
        elif k % 4 == 2:
            cut = at + int(rng.randint(1, 8))
            out.append(("cut%d" % cut, s[:cut]))
        else:
            ins = at + int(rng.randint(3, 8))
            out.append(("ins%d" % ins, s[:ins] + bytes([int(rng.randint(0, 256))]) + s[ins:]))
    return out
