"""Motion vectors at every f_code in the interlaced decode units, on the CPU: dec::bp_component, dec::il_field_vector, dec::t_dual_prime
and dec::chroma_vector of csrc/m2v_decode_kernels.hpp compiled with g++ against tests/vec_ref.py, a second statement of 7.6.3 that
parses nothing; every stream of tests/vec_cases.py through vec_ref (the vectors from the codes the writer logged, the frames from the
references that take absolute vectors), through decoder.decode and through the g++ host builds of the decode units - byte for byte,
record for record; what the streams reach, asserted from the writers' logs alone; every wrong form of vec_ref shown to change a case;
literal pictures; the refusals with their offsets.  tests/test_gpu_decode_vectors.py runs the same streams on the device."""
import numpy as np
import pytest

import dec_cases as D
import vec_cases as V
import vec_ref as VR

M = D.M


def flat(frames):
    return np.stack([np.concatenate([p.reshape(-1) for p in f]) for f in frames])


def predictors(f_code):
    """both ends of the range, around zero, and with them every negative odd value within 3 of those"""
    f = 1 << (f_code - 1)
    return sorted({-16 * f + k for k in range(4)} | {16 * f - 1 - k for k in range(4)} | set(range(-3, 4)))


def residuals(f_code):
    f = 1 << (f_code - 1)
    return sorted({0, f // 2, f - 1})


# ---- the functions ----
@pytest.mark.parametrize("f_code", range(1, 10))
def test_component_every_f_code(f_code):
    """dec::bp_component for every motion code, residuals 0, f / 2 and f - 1, predictors at both ends of the range and around zero:
    the vector is 7.6.3.1's, and both wraps are reached"""
    wraps = set()
    for pmv in predictors(f_code):
        for code in range(-16, 17):
            for residual in residuals(f_code):
                want = VR.component(pmv, code, residual, f_code)
                wraps.add(VR.wrapped(pmv + VR.delta_of(code, residual, f_code), f_code)[1])
                assert V.host_component(pmv, code, residual, f_code) == want, (pmv, code, residual)
    assert wraps == {-1, 0, 1}


@pytest.mark.parametrize("f_code", range(1, 10))
def test_field_vector_every_f_code(f_code):
    """dec::il_field_vector: the vertical component from the predictor DIV 2 - toward minus infinity: the predictors include every
    negative odd value near the ends and near zero - with the range test on the halved scale, the predictor left behind twice the
    vector; the horizontal component with its own f_code, which differs"""
    fh = 10 - f_code if f_code != 5 else 3
    wraps, odd = set(), 0
    for pmv in predictors(f_code):
        for code in range(-16, 17):
            for residual in residuals(f_code):
                hc = ((code + 5) % 33 - 16, (residual * 3 + 1) % (1 << (fh - 1)))
                v, left = V.host_field_vector((pmv // 3, pmv), (hc, (code, residual)), (fh, f_code))
                vy, py, k = VR.field_component(pmv, code, residual, f_code)
                vx = VR.component(pmv // 3, hc[0], hc[1], fh)
                assert (v, left) == ((vx, vy), (vx, py)), (pmv, code, residual)
                assert py == 2 * vy
                wraps.add(k)
                odd += pmv < 0 and pmv & 1 and vy != VR.field_component(pmv, code, residual, f_code, "half_toward_zero")[0]
    assert wraps == {-1, 0, 1} and odd > 0
    # the wrong forms differ from it where they should: the range test on the doubled value at the top of the halved range
    f = 1 << (f_code - 1)
    assert VR.field_component(16 * f - 2, 1, 0, f_code)[0] == 8 * f and VR.field_component(16 * f - 2, 1, 0, f_code, "wrap_on_doubled")[0] == -8 * f


def test_dual_prime_against_the_rule():
    """dec::t_dual_prime for every vx, vy in [-64, 64] and at both ends of f_code 9's ranges, all nine dmvectors, both top_field_first"""
    ends = [-4096, -4095, -2048, -2047, 2046, 2047, 4094, 4095]
    values = list(range(-64, 65))
    pairs = [(x, y) for x in values for y in values] + [(x, y) for x in ends for y in ends] + [(x, y) for x in ends for y in (-3, 0, 5)]
    rows = [(x, y, d0, d1, tff) for x, y in pairs for d0 in (-1, 0, 1) for d1 in (-1, 0, 1) for tff in (0, 1)]
    got = V.host_dual_prime(rows)
    assert len(rows) >= 129 * 129 * 18
    for (x, y, d0, d1, tff), g in zip(rows, got.tolist()):
        t, b = VR.dual_frame((x, y), (d0, d1), tff)
        assert g == [x, y, x, y, t[0], t[1], b[0], b[1], 0, 1, 1, 0], (x, y, d0, d1, tff)


# typed by hand from 7.6.3.6: (vx, vy, dmvector, top_field_first) -> the vector for the top-field lines (from the bottom field), the
# vector for the bottom-field lines (from the top field).  3 // 2 = 2, 5 // 2 = 3, 9 // 2 = 5, 15 // 2 = 8, and their negatives
DUAL_ROWS = (((3, 5), (1, 1), 1, (3, 3), (6, 10)),
             ((3, 5), (1, 1), 0, (6, 8), (3, 5)),
             ((-3, -5), (0, 0), 1, (-2, -4), (-5, -7)),
             ((-3, -5), (0, 0), 0, (-5, -9), (-2, -2)),
             ((4, -2), (-1, 1), 1, (1, -1), (5, -1)),
             ((1, -1), (0, -1), 0, (2, -4), (1, -1)))


def test_dual_prime_literal_rows():
    for v, dmv, tff, t, b in DUAL_ROWS:
        assert VR.dual_frame(v, dmv, tff) == (t, b), (v, dmv, tff)
        assert V.host_dual_prime([(v[0], v[1], dmv[0], dmv[1], tff)])[0].tolist()[4:8] == [t[0], t[1], b[0], b[1]]
    # a field picture: one vector, the factor 1, e by the parity
    assert VR.dual_field((3, 5), (1, 1), 0) == (3, 3) and VR.dual_field((3, 5), (1, 1), 1) == (3, 5)
    assert VR.dual_field((-3, -5), (0, -1), 0) == (-2, -5) and VR.dual_field((-3, -5), (0, -1), 1) == (-2, -3)


def test_half_and_chroma():
    L = V.host_lib()
    for a in range(-12300, 12300):
        assert L.vec_host_half(a) == VR.half(a)
    for v in range(-4096, 4096):
        assert L.vec_host_chroma(v) == VR.chroma(v)
    assert VR.chroma(-4095) == -2047 and VR.chroma(-4095, "chroma_shift") == -2048 and VR.half(-3) == -2 and VR.half(3) == 2


def test_walk_skipped_macroblocks():
    """the rules no stream of frame pictures here carries, on a log typed by hand: a P picture's skipped macroblock resets the
    predictors, a B picture's takes PMV[0][s] in the directions in front and leaves them"""
    mb = lambda col, **kw: dict(dict(row=0, col=col, intra=False, nomc=False, skip=False, motion="frame", fwd=None, bwd=None), **kw)
    codes = [(1, 5, 0), (1, -3, 0), (1, 2, 0), (1, 1, 0)]
    log = dict(pictures=[dict(type=2, f_code=(1, 1, 1, 1), mbs=[mb(0, fwd=(5, -3)), mb(1, skip=True), mb(2, fwd=(2, 1))])], writer=dict(codes=codes))
    assert VR.vectors(log)[0] == [(0, 0, (5, -3), None, None), (0, 1, (0, 0), None, None), (0, 2, (2, 1), None, None)]
    codes = [(1, 5, 0), (1, -3, 0), (1, 2, 0), (1, 1, 0), (1, 1, 0), (1, 1, 0), (1, 0, 0), (1, -1, 0)]
    log = dict(pictures=[dict(type=3, f_code=(1, 1, 1, 1), mbs=[mb(0, fwd=(5, -3), bwd=(2, 1)), mb(1, skip=True), mb(2, fwd=(6, -2), bwd=(2, 0))])], writer=dict(codes=codes))
    assert VR.vectors(log)[0] == [(0, 0, (5, -3), (2, 1), None), (0, 1, (5, -3), (2, 1), None), (0, 2, (6, -2), (2, 0), None)]


# ---- the streams ----
@pytest.mark.parametrize("name", V.NAMES)
def test_streams(name):
    """vec_ref's vectors are the ones the case described; its frames are the definition's; the g++ build of the case's unit gives the
    same bytes and the same record; the definition with "decode_join" 3 gives the same frames"""
    c = V.get(name)
    told = [[(m["row"], m["col"], m["fwd"], m["bwd"]) for m in p["mbs"] if not m.get("skip") and not m["intra"] and not m["nomc"]] for p in c["log"]["pictures"]]
    read = [[(m["row"], m["col"], m["fwd"], m["bwd"]) for m in p["mbs"] if not m.get("skip") and not m["intra"] and not m["nomc"]] for p in VR.walk(c["log"])[0]]
    assert read == told
    d, at = V.spec_cached(c["stream"], V.options(c))
    assert d is not None, at
    want = D.frames_of(d)
    assert np.array_equal(flat(V.ref_frames(name)), want)
    f, r = V.host_decode(c)
    assert r["status"] == D.OK and np.array_equal(f, want)
    rec = V.record_of(d, c["stream"])
    assert {k: r[k] for k in rec} == rec and r["out_bytes"] == r["pictures"] * r["frame_bytes"]
    for unit, o, join in V.ladder(c)[1:]:
        dd, at = V.spec_cached(c["stream"], o, join)
        assert dd is not None and np.array_equal(D.frames_of(dd), want), unit


def test_batch_names():
    """the streams the device decodes in chunks of one and two frames: those with B pictures or field pictures"""
    assert V.BATCH_NAMES == tuple(n for n in V.NAMES if V.get(n)["needs"] in ("b", "f", "fb"))


def reached(name, **where):
    """the (f_code, wrap) of the components of the case's trace with the given fields"""
    return {(x["f_code"], x["wrap"]) for x in V.trace(name) if all(x[k] == v for k, v in where.items())}


def both_wraps(name, f_codes, **where):
    got = reached(name, **where)
    missing = [(f, k) for f in f_codes for k in (-1, 1) if (f, k) not in got]
    assert not missing, (name, where, missing)


def every_f_code_has_a_residual(name):
    tr = V.trace(name)
    named = {f for p in V.get(name)["log"]["pictures"] if p["type"] != 1 or p.get("cmv") for f in p["f_code"][:4 if p["type"] == 3 else 2]}
    assert {x["f_code"] for x in tr if x["residual"]} == {f for f in named if f > 1}, name
    assert {x["f_code"] for x in tr} == named, name


def test_coverage_frame_pictures():
    """from the writers' logs alone: what the streams of frame pictures reach"""
    for name in ("il_fcodes", "il_fcodes_wide", "il_fcodes_tall", "il_halved_wrap", "wide_2048"):
        every_f_code_has_a_residual(name)
    # il_fcodes: frame-based and field-based alternate, every field vector behind a frame vector and the reverse
    for name in ("il_fcodes", "il_fcodes_wide", "il_fcodes_tall"):
        for p in V.get(name)["log"]["pictures"][1:]:
            for a, b in zip(p["mbs"], p["mbs"][1:]):
                assert b["col"] == 0 or {a["motion"], b["motion"]} == {"frame", "field"}
    for mode in ("frame", "field"):
        both_wraps("il_fcodes", range(1, 6), mode=mode, s=0, t=0)
        both_wraps("il_fcodes", range(2, 6), mode=mode, s=1, t=0)
    both_wraps("il_fcodes", range(1, 5), mode="frame", s=0, t=1)
    both_wraps("il_fcodes", range(1, 5), mode="frame", s=1, t=1)
    fcs = [p["f_code"] for p in V.get("il_fcodes")["log"]["pictures"] if p["type"] == 3]
    assert fcs and all(len(set(f)) == 4 for f in fcs) and max(max(f) for f in fcs) == 5
    # a field vector's vertical predictor that a frame vector left negative and odd: DIV 2 and / 2 differ
    for name, least in (("il_fcodes", 100), ("il_fcodes_wide", 100), ("il_fcodes_tall", 100)):
        odd = [x for x in V.trace(name) if x["mode"] == "field" and x["t"] == 1 and x["pmv"] < 0 and x["pmv"] & 1]
        assert len(odd) >= least and all(x["pred"] == (x["pmv"] - 1) // 2 for x in odd), name
        assert {x["f_code"] for x in odd} == {x["f_code"] for x in V.trace(name) if x["t"] == 1}
    # the field vector itself stays inside Table 7-8's halved range there, so its sum never wraps
    for name in ("il_fcodes", "il_fcodes_wide", "il_fcodes_tall", "wide_2048"):
        assert all(x["wrap"] == 0 and -8 << (x["f_code"] - 1) <= x["vector"] < 8 << (x["f_code"] - 1) for x in V.trace(name) if x["mode"] == "field" and x["t"] == 1)
    # il_fcodes_wide: field-based horizontal wraps at f_codes 6 to 8, forward and backward; f_code 9 with deltas past 2048 and no wrap
    for s in (0, 1):
        both_wraps("il_fcodes_wide", (6, 7, 8), mode="field", s=s, t=0)
        both_wraps("il_fcodes_wide", (6, 7, 8), mode="frame", s=s, t=0)
        nine = [x for x in V.trace("il_fcodes_wide") if x["f_code"] == 9 and x["s"] == s]
        assert nine and all(x["wrap"] == 0 for x in nine) and max(abs(x["vector"] - x["pred"]) for x in nine) > 2048
        assert max(x["vector"] for x in nine) > 2047 and min(x["vector"] for x in nine) < -2048      # more than twelve bits hold
    # il_fcodes_tall: vertical f_codes 5 to 7, frame-based with both wraps, field-based with residuals
    for s in (0, 1):
        both_wraps("il_fcodes_tall", (5, 6, 7), mode="frame", s=s, t=1)
        assert {x["f_code"] for x in V.trace("il_fcodes_tall") if x["mode"] == "field" and x["t"] == 1 and x["s"] == s and x["residual"]} == {5, 6, 7}
    # il_halved_wrap: the wrap on the halved scale, vertical f_codes 1 to 3; the vectors lie outside the halved range
    both_wraps("il_halved_wrap", (1, 2, 3), mode="field", t=1)
    assert all(not -8 << (x["f_code"] - 1) <= x["vector"] < 8 << (x["f_code"] - 1) for x in V.trace("il_halved_wrap") if x["mode"] == "field" and x["t"] == 1 and x["wrap"])
    # wide_2048: the longest displacement f_code 9 allows in this width, both signs, in both directions; the other parity
    far = [x["vector"] for x in V.trace("wide_2048") if x["t"] == 0]
    assert max(far) == 32 * 127 and min(far) == -32 * 127 + 1      # column 0 reads column 127, column 127 reads column 0 with a half sample
    for s in (0, 1):
        far = [x["vector"] for x in V.trace("wide_2048") if x["s"] == s and x["t"] == 0]
        assert max(far) >= 32 * 126 and min(far) <= -32 * 126
    c = V.get("wide_2048")
    assert (c["log"]["w"], c["log"]["h"]) == (2048, 32)
    for p in c["log"]["pictures"][1:]:
        selects = [(v[0][0], v[1][0]) for m in p["mbs"] for v in (m["fwd"], m["bwd"]) if v is not None]
        assert set(selects) == {(1, 0), (0, 1)} and 3 * selects.count((1, 0)) >= len(selects)      # (1, 0): either half reads the other parity
        assert all(m["motion"] == "field" for m in p["mbs"]) and sum(m["cbp"] != 0 for m in p["mbs"]) <= 8


def test_coverage_dual_prime_and_concealment():
    for name, tff, most in (("dual_far", 1, 5), ("dual_far_bff", 0, 5), ("dual_far_wide", 1, 8), ("dual_far_bff_wide", 0, 8)):
        c = V.get(name)
        every_f_code_has_a_residual(name)
        L = c["log"]["writer"]
        assert {d[4] for d in L["duals"]} == set(V.NINE) and {d[5] for d in L["duals"]} == {tff}
        assert max(x["f_code"] for x in V.trace(name) if x["mode"] == "dual") == most
        mbw, rows = c["log"]["mbw"], c["log"]["rows"]
        edges = set()
        for p in VR.walk(c["log"])[0]:
            for m in p["mbs"]:
                if m.get("motion") != "dual" or m["intra"]:
                    continue
                for vx, vy in (m["fwd"][0],) + tuple(m["derived"]):
                    x0, y0 = 16 * m["col"] + (vx >> 1), 8 * m["row"] + (vy >> 1)
                    edges |= {e for e, hit in (("left", x0 == 0), ("right", x0 + 15 + (vx & 1) == 16 * mbw - 1), ("top", y0 == 0), ("bottom", y0 + 7 + (vy & 1) == 8 * rows - 1)) if hit}
        assert edges == {"left", "right", "top", "bottom"}, (name, edges)
        for t in (0, 1):
            vs = [x["vector"] for x in V.trace(name) if x["mode"] == "dual" and x["t"] == t]
            assert {(v > 0, v & 1) for v in vs if v} == {(a, b) for a in (False, True) for b in (0, 1)}, (name, t)
        # a dual-prime macroblock behind a frame vector with a negative odd vertical component: its prediction is the floor
        assert any(x["mode"] == "dual" and x["t"] == 1 and x["pmv"] < 0 and x["pmv"] & 1 for x in V.trace(name)), name
    c = V.get("conceal_fcodes")
    every_f_code_has_a_residual("conceal_fcodes")
    tr = [x for x in V.trace("conceal_fcodes") if x["mode"] == "conceal"]
    assert tr and all(x["code"] != 0 and x["residual"] != 0 for x in tr), "every concealment vector has a residual that is not zero"
    assert {(x["pic"], x["t"], x["f_code"]) for x in tr} == {(0, 0, 4), (0, 1, 3), (1, 0, 7), (1, 1, 5), (2, 0, 4), (2, 1, 3)}
    both_wraps("conceal_fcodes", (4, 7), mode="conceal", t=0)
    both_wraps("conceal_fcodes", (3, 5), mode="conceal", t=1)
    for p in c["log"]["pictures"][1:]:
        assert p["cmv"] == 1 and all(m["intra"] == (m["col"] % 2 == 0) for m in p["mbs"])      # every vector stands behind a concealment vector
    assert len(c["log"]["writer"]["b15"]) > 20 and c["log"]["writer"]["kept"] > 0


def test_coverage_field_pictures():
    for name in ("fld_fcodes", "fld_fcodes_tall", "wide_2048_fields"):
        every_f_code_has_a_residual(name)
    L = V.get("fld_fcodes")["log"]["writer"]
    for ptype in (2, 3):
        assert {(f["ps"], f["second"]) for f in L["fields"] if f["type"] == ptype} == {(1, False), (1, True), (2, False), (2, True)}
    modes = {m["motion"] for m in L["fmbs"] if m.get("motion")}
    assert modes == {"field", "16x8", "dual"}
    for mode in ("field", "16x8"):
        both_wraps("fld_fcodes", range(1, 6), mode=mode, s=0, t=0)
        both_wraps("fld_fcodes", range(1, 4), mode=mode, s=0, t=1)
        both_wraps("fld_fcodes_tall", range(4, 8), mode=mode, s=0, t=1)
        both_wraps("fld_fcodes", (2, 4), mode=mode, s=1, t=0)      # backward, in the B fields
        both_wraps("fld_fcodes", range(1, 4), mode=mode, s=1, t=1)
        both_wraps("fld_fcodes_tall", (5, 7), mode=mode, s=1, t=1)
    assert {x["f_code"] for x in V.trace("fld_fcodes") if x["mode"] == "dual" and x["t"] == 0} == {2, 3, 4, 5}
    # the two vectors of a 16 x 8 macroblock wrap on their own
    for name in ("fld_fcodes", "fld_fcodes_tall"):
        pairs = {}
        for x in V.trace(name):
            if x["mode"] == "16x8":
                pairs.setdefault((x["pic"], x["row"], x["col"], x["s"], x["t"]), {})[x["r"]] = x["wrap"]
        assert any(p[0] and not p[1] for p in pairs.values()) and any(p[1] and not p[0] for p in pairs.values()), name
    # dual prime in both parities (e -1 and +1) with reads at the field's edges
    for name in ("fld_fcodes", "fld_fcodes_tall"):
        c = V.get(name)
        mbw, rows = c["log"]["mbw"], c["log"]["rows"]
        edges = set()
        for p in VR.walk(c["log"])[0]:
            for m in p["mbs"]:
                if m.get("motion") != "dual":
                    continue
                for vx, vy in (m["fwd"][0], m["derived"]):
                    x0, y0 = 16 * m["col"] + (vx >> 1), 16 * m["row"] + (vy >> 1)
                    edges |= {(p["ps"], e) for e, hit in (("left", x0 == 0), ("right", x0 + 15 + (vx & 1) == 16 * mbw - 1), ("top", y0 == 0), ("bottom", y0 + 15 + (vy & 1) == 16 * rows - 1)) if hit}
        assert {ps for ps, e in edges} == {1, 2} and {e for ps, e in edges} >= ({"top", "bottom"} if mbw == 2 else {"left", "right", "top", "bottom"}), (name, edges)
    # the second P field of the stream's first frame reads its first field, the only one there
    first = [m for m in L["fmbs"] if m["pic"] == 1 and m.get("motion") in ("field", "16x8")]
    par = L["fields"][0]["ps"] - 1
    assert L["fields"][1]["second"] and L["fields"][1]["type"] == 2 and first
    assert all(sel == par for m in first for sel in ([m["fwd"][0]] if m["motion"] == "field" else [m["fwd"][0][0], m["fwd"][1][0]]))
    far = [x["vector"] for x in V.trace("wide_2048_fields") if x["t"] == 0]
    assert max(far) == 32 * 127 and min(far) == -32 * 127 + 1


# ---- the wrong forms ----
def test_every_wrong_form_changes_a_case(capsys):
    """each wrong form of vec_ref changes the frames of the case named for it (or leaves the picture there: a decoder with that mistake
    refuses a stream the definition accepts); "=" marks a case whose vectors the form cannot change"""
    assert set(V.CATCHES) == set(VR.WRONG)
    lines = [" " * 30 + " ".join(n[:9].ljust(9) for n in V.NAMES)]
    for w in VR.WRONG:
        row = {n: V.changed(n, w) for n in V.NAMES}
        lines.append(w.ljust(30) + " ".join(row[n].ljust(9) for n in V.NAMES))
        assert row[V.CATCHES[w]] in ("X", "O"), (w, V.CATCHES[w], row)
    with capsys.disabled():
        print("\n" + "\n".join(lines))


# ---- literal pictures and refusals ----
@pytest.mark.parametrize("name", sorted(V.known()))
def test_known_answers(name):
    k = V.known()[name]
    want = flat(k["frames"])
    for unit, o, join in V.ladder(k):
        d, at = V.spec_cached(k["stream"], o, join)
        assert d is not None and np.array_equal(D.frames_of(d), want), (name, unit, at)
    f, r = V.host_decode(k)
    assert r["status"] == D.OK and np.array_equal(f, want)


@pytest.mark.parametrize("name", sorted(V.refusals()))
def test_refusals(name):
    """the component is inside its f_code's range and the read is not: refused at the slice, by the definition under every option set
    and by the g++ build"""
    r = V.refusals()[name]
    for unit, o, join in V.ladder(r):
        assert V.spec_cached(r["stream"], o, join) == (None, r["offset"]), (name, unit)
    f, rec = V.host_decode(r)
    assert f is None and (rec["status"], rec["err_offset"], rec["out_bytes"]) == (D.SYNTAX, r["offset"], 0)
