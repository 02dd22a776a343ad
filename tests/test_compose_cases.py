"""CPU: the model of tests/compose_cases.py before tests/test_gpu_compose.py relies on it.  With one feature set it reproduces what the
older case modules state for their own cases; every expected stream of pairs() and maximal() is read by decoder.py - picture count and
types, GOP starts, sizes, frame rate and colour codes are the call's, the decoded pictures are the expected reconstruction (a standard
decoder with "conformant", the module's own loop without), every container's payload read back is the clip's stream; no legal pair of
levels is missing from the rows; and the comparison the GPU test uses rejects every altered expectation and names what was altered.

Measured on the development machine (the tests print the figures): pairs() has 27 rows for 772 legal pairs of
levels, port_pairs() 19 for 300; the 51 cases of this module run in 26 s, 21 s of which decoder.py spends on the 30 expected streams."""
import time

import numpy as np
import pytest

import compose_cases as C
import test_container as TC

M, D, F, G, Q, R, S, SC, X = C.M, C.D, C.F, C.G, C.Q, C.R, C.S, C.SC, C.X
T0 = time.time()


def tup(d):
    return tuple(sorted(d.items()))


def material(name, frames):
    C.MATERIAL[name] = np.ascontiguousarray(frames).reshape(len(frames), -1)
    return name


def same_records(got, want):
    assert got.dtype == want.dtype and len(got) == len(want), (len(got), len(want))
    for k in want.dtype.names:
        assert np.array_equal(got[k], want[k]), (k, got[k].tolist(), want[k].tolist())


# ---- agreement with the older modules ----
def test_agrees_with_seq_cases():
    c = Q.comp()
    ln, pf = tuple(c["lengths"]), c["pf"]
    base = dict(material=material("seq_comp", c["frames"]), geom=(c["W"], c["H"], None), pf=pf, seqs=ln)
    want, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], pf)
    e = C.expected(C.call(**base))
    assert e["stream"] == want and e["offsets"] == off
    same_records(e["sequence_report"], Q.records(c["lengths"], off, pf))
    for name in ("gop_report", "scene_report", "picture_stats", "mux_report"):
        assert len(e[name]) == 0
    assert C.expected(C.call(rate=("sched", (1, 4, 3)), vlq=(3, 1), **base))["stream"] == Q.levels_expected([1, 4, 3])[0]
    d = D.desc(frame_rate_code=4, repeat_headers=1)
    assert C.expected(C.call(desc=tup(d), **base))["stream"] == Q.desc_expected(d)[0]
    same_records(C.expected(C.call(stats=1, **base))["picture_stats"], Q.stats_expected())
    assert np.array_equal(C.expected(C.call(recon="nv12", **base))["recon"], Q.recon_expected("nv12"))
    assert C.expected(C.call(conformant=1, **base))["stream"] == Q.expected(c["frames"], c["lengths"], c["W"], c["H"], pf, conformant=True)[0]


def test_agrees_with_scene_cases_and_desc_cases():
    f, W, H = G.clip_args("c96")
    cuts = SC.cuts_of(f, 3000)
    assert cuts == [4, 8]
    base = dict(material=material("c96", f), geom=(W, H, None), pf=3)
    e = C.expected(C.call(layout=("starts", (5,), 3000), rate=("sched", (1, 4, 3)), **base))
    assert e["stream"] == SC.expected(f, W, H, 3, [5], levels=[1, 4, 3], cuts=cuts)
    same_records(e["scene_report"], SC.records(len(f), 3, [5], cuts, SC.diffs(f)))
    e = C.expected(C.call(layout=("starts", (2, 7), 0), **base))
    assert e["stream"] == SC.expected(f, W, H, 3, [2, 7]) == R.starts_case()["stream"]
    same_records(e["scene_report"], SC.records(len(f), 3, [2, 7]))
    assert np.array_equal(C.expected(C.call(layout=("starts", (2, 7), 0), recon="i420", **base))["recon"],
                          R.write_layout(R.starts_case()["recon"], W, H, "i420"))
    # a description: the plain stream rewritten, and with list and detector
    plain = G.encoded(f, W, H, 2, 2)[0]
    d = D.desc(repeat_headers=1, frame_rate_code=5, colour_primaries=1, transfer_characteristics=1, matrix_coefficients=1)
    assert C.expected(C.call(desc=tup(d), **dict(base, pf=2)))["stream"] == D.described(plain, D.cadence(len(f), 2), d)
    assert C.expected(C.call(**dict(base, pf=2)))["stream"] == plain
    want = D.described(SC.expected(f, W, H, 3, [5], cuts=cuts), [0, 4, 5, 8], d)
    assert C.expected(C.call(desc=tup(d), layout=("starts", (5,), 3000), **base))["stream"] == want


def test_agrees_with_gop_cases():
    f, W, H = G.clip_args("c80")
    base = dict(material=material("c80", f), geom=(W, H, None), pf=2)
    assert C.expected(C.call(rate=("sched", tuple(G.SCHEDULE)), **base))["stream"] == G.splice(f, W, H, 2, G.SCHEDULE)
    for name in ("b3500", "b3552", "b3551", "b800", "sched"):
        cc = G.cap_case(name)
        rate = ("cap", cc["B"], tuple(cc["sched"])) if cc["sched"] else ("cap", cc["B"])
        e = C.expected(C.call(rate=rate, vlq=(3, cc["Q"]), **base))
        assert e["stream"] == cc["stream"], name
        same_records(e["gop_report"], cc["records"])
    # with repeated headers the cap's bytes do not count the copies
    cc = G.cap_case("b3500")
    d = D.desc(repeat_headers=1)
    e = C.expected(C.call(rate=("cap", cc["B"]), vlq=(3, cc["Q"]), desc=tup(d), **base))
    same_records(e["gop_report"], cc["records"])
    assert e["stream"] == D.described(cc["stream"], D.cadence(len(f), 2), d) and len(e["stream"]) > len(cc["stream"])
    assert np.array_equal(C.expected(C.call(rate=("cap", cc["B"]), vlq=(3, cc["Q"]), recon="i420", **base))["recon"],
                          R.write_layout(R.cap_case()["recon"], W, H, "i420"))


@pytest.mark.parametrize("kind", ["444", "i420", "nv12", "rgb24", "rgbp"])
def test_agrees_with_fit_cases(kind):
    w, h, n, pf = 100, 70, 4, 2
    x = F.source(w, h, n, kind, seed=3)
    mat = "bt709" if kind == "rgbp" else "bt601"
    want = F.want_stream(x, w, h, kind, pf, (6, 6, 3, 2), mat)
    name = material("fit_" + kind, x)
    assert C.expected(C.call(material=name, geom=(w, h, "module"), kind=kind, pf=pf))["stream"] == want
    assert C.expected(C.call(material=name, geom=(w, h, "true"), kind=kind, pf=pf))["stream"] == M.set_header_size(want, w, h)


def test_agrees_with_recon_cases_and_stats_cases():
    c = R.fit_case(100, 70, "i420")
    base = dict(material=material("recon_fit", c["x"]), geom=(100, 70, "true"), kind="i420", pf=c["pf"])
    e = C.expected(C.call(recon="nv12", stats=1, **base))
    assert np.array_equal(e["recon"], R.write_layout(c["recon"], c["W"], c["H"], "nv12", c["region"]))
    s = S.fit_case("fit420")
    e = C.expected(C.call(stats=1, **dict(base, material=material("stats_fit", s["x"]), pf=s["pf"])))
    same_records(e["picture_stats"], s["records"])
    assert e["stream"] == M.set_header_size(s["stream"], 100, 70)
    s = S.case("conformant")
    e = C.expected(C.call(material=material("stats_conf", s["frames"]), geom=(s["W"], s["H"], None), pf=s["pf"], stats=1, conformant=1))
    same_records(e["picture_stats"], s["records"])
    assert e["stream"] == s["stream"]


# ---- the rows ----
def rows():
    out = [(C.name_of(r), r) for r in C.pairs()]
    out += [(k, r) for k, r in sorted(C.maximal().items())]
    return out


def test_every_legal_pair_of_levels_is_in_a_row():
    for factors, (got, every), excluded in ((C.FACTORS, C._pairs(), C.EXCLUDED), (C.PORT_FACTORS, C._port_pairs(), ())):
        assert all(C.legal(r) for r in got)
        covered = set().union(*[C.pairs_of(r, factors) for r in got])
        assert every <= covered, sorted(every - covered)
        # the pairs left out are exactly the table's: every other pair of levels is in `every`
        names = {((factors[i][0], factors[i][1][a]), (factors[j][0], factors[j][1][b]))
                 for i in range(len(factors)) for j in range(i + 1, len(factors)) for a in range(len(factors[i][1]))
                 for b in range(len(factors[j][1])) if ((i, a), (j, b)) not in every}
        assert names == {tuple(sorted(p, key=lambda fl: [f for f, _ in factors].index(fl[0]))) for p in excluded}, names
    assert C.pairs() == C.pairs() and C.port_pairs() == C.port_pairs()            # deterministic
    # the port path's refusals: every level the table names makes a port call illegal
    for f, v in C.PORT_EXCLUDED:
        assert not C.legal(C.call(entry="port", **{f: v}))
    for r in C.maximal().values():
        assert C.legal(r)
    print("pairs(): %d rows for %d legal pairs, port_pairs(): %d rows for %d" % (len(C._pairs()[0]), len(C._pairs()[1]),
                                                                                 len(C._port_pairs()[0]), len(C._port_pairs()[1])))


def test_the_cap_and_the_threshold_do_what_they_are_chosen_for():
    seen_again = 0
    for name, r in rows() + [(C.name_of(r), r) for seed, vlq in C.SESSIONS for r in C.session(seed, vlq)]:
        e = C.expected(r)
        if r["rate"] == "cap":
            tries, Qh = e["gop_report"]["tries"], r["vlq"][1]
            assert tries.min() == 1, name                                   # at least one GOP is not coded again
            if Qh < 4:                                                      # (a handle at level 4 has nowhere to go: tries are 1)
                assert tries.max() > 1 and (e["gop_report"]["level"] > Qh).any(), name
                seen_again += 1
            else:
                assert tries.max() == 1 and e["gop_report"]["over"].any(), name
            if r["desc"] == "repeat":                                       # the copies are not counted: B judges the GOP alone
                sizes = [len(g) for g in G.cut(C.expected(dict(r, desc=None))["stream"])[1]]
                assert e["gop_report"]["bytes"].tolist() == sizes, name
                assert len(e["stream"]) >= sum(sizes) + 34 * len(sizes), name
        if r["layout"] in ("cut", "both"):
            fl = e["scene_report"]["flags"]
            assert [int(n) for n in np.flatnonzero(fl & SC.CUT)] == [5, 10], name
            assert (fl[[5, 10]] == SC.CUT).any(), name                     # a flagged frame off the cadence and off the list
            assert not set(C.LIST) & {5, 10}
    assert seen_again >= 4 and C.maximal()["cap"]["vlq"][1] < 4


@pytest.mark.parametrize("seed,vlq", C.SESSIONS)
def test_session_order(seed, vlq):
    calls = C.session(seed, vlq)
    assert all(c["vlq"] == vlq for c in calls)
    fewest, on, changed, off = C.session_facts(calls)
    assert len(calls) == 12 and fewest >= 4 and on >= C.ONOFF and off >= C.ONOFF and changed >= C.CHANGEABLE
    assert [c["geom"][:2] for c in calls] == [(96, 64)] * 3 + [(100, 70)] * 3 + [(64, 64)] * 3 + [(96, 64)] * 3
    assert [c["entry"] for c in calls] == ["block", "begin"] * 6 and all(C.legal(c) for c in calls)
    assert calls == C.session(seed, vlq)


# ---- an independent reading: decoder.py and the demultiplexers ----
@pytest.mark.parametrize("name,r", rows(), ids=[n for n, _ in rows()])
def test_decoder_reads_the_expected_stream(name, r):
    w, h, header = r["geom"]
    W, H = F.padded(w, h)
    pf = r["pf"]
    e = C.expected(dict(r, recon="i420"))
    assert e["stream"] == C.expected(r)["stream"]
    d = C.desc_of(r)
    starts, cuts = C.starts_of(r), [int(n) for n in np.flatnonzero(e["scene_report"]["flags"] & SC.CUT)] if len(e["scene_report"]) else []
    rec_y, rec_u, rec_v = M.planes_of_recon(e["recon"], w if header else W, h if header else H, "i420")
    f0 = 0
    for b, (s, n) in enumerate(zip(e["clips"], e["lengths"])):
        dec = M.decoder.decode(s, quirks=not r["conformant"])
        flags = SC.layout(n, pf, starts, cuts)
        assert len(dec.pictures) == n and [p["type"] for p in dec.pictures] == [1 if fl else 2 for fl in flags]
        gop_at = [k for k, fl in enumerate(flags) if fl]
        assert len(dec.gops) == len(gop_at)
        F_ = D.RATE[d["frame_rate_code"]]
        assert [(g["seconds"], g["pictures"]) for g in dec.gops] == [(k // F_, k % F_) for k in gop_at]
        assert (dec.width, dec.height) == ((w, h) if header == "true" else (W, H))
        q = dec.sequence
        assert q["display_size"] == (dec.width, dec.height) and q["frame_rate_code"] == d["frame_rate_code"]
        assert (q["colour_primaries"], q["transfer_characteristics"], q["matrix_coefficients"]) == \
            (d["colour_primaries"], d["transfer_characteristics"], d["matrix_coefficients"])
        assert (q["aspect"], q["bit_rate"], q["vbv"]) == (d["aspect_ratio_information"], d["bit_rate_400"], d["vbv_buffer_size_16k"])
        assert dec.repeated_headers == (len(gop_at) - 1 if d["repeat_headers"] else 0)
        # the level of every slice: the schedule's or the cap's
        if len(e["gop_report"]):
            lv = e["gop_report"]["level"].tolist()
        else:
            lv = G.per_gop(C.levels_of(r), len(gop_at)) if C.levels_of(r) else [r["vlq"][1]] * len(gop_at)
        at = np.cumsum([1 if fl else 0 for fl in flags]) - 1
        assert dec.slice_qcodes == [[1 << lv[at[k]]] * (H // 16) for k in range(n)]
        # the pictures: what the expected reconstruction buffer holds (cropped where a size is set)
        ww, hh = (w, h) if header else (W, H)
        for k in range(n):
            y, u, v = dec.frames[k]
            assert np.array_equal(y[:hh, :ww], rec_y[f0 + k]) and np.array_equal(u[:(hh + 1) // 2, :(ww + 1) // 2], rec_u[f0 + k]) \
                and np.array_equal(v[:(hh + 1) // 2, :(ww + 1) // 2], rec_v[f0 + k]), (name, b, k)
        f0 += n
        # the containers' payload is the clip's stream
        info, pics = X.C.scan(s)
        assert info.pictures == n and info.gops == len(gop_at) and info.frame_rate_code == d["frame_rate_code"]
        if r["mux"]:
            got = (TC.demux_ts if r["mux"] == "ts" else TC.demux_ps)(C.expected(r)["containers"][b])
            assert got[0] == s[:info.bytes], (name, b)


# ---- the checker can fail ----
def altered(c, what):
    """render(call) with one thing altered -> (got, want, the item check() has to name)"""
    want = C.expected(c)
    got = C.render(c)
    if what == "time code":
        o = [m for m in want["marks"] if m[2].startswith("time code")][-1][0]
        got["stream_buf"][o + 2] ^= 0x20
        return got, want, "stream"
    if what == "record field":
        name = [n for n in C.REPORTS if len(want[n])][altered.turn % len([n for n in C.REPORTS if len(want[n])])]
        altered.turn += 1
        field = want[name].dtype.names[-2]
        got[name][field][-1] += 1
        return got, want, "%s.%s" % (name, field)
    if what == "recon inside":
        got["recon_buf"][want["recon"].size - 1] ^= 1                        # the last sample of the last frame's crop
        return got, want, "recon"
    if what == "recon outside":
        got["recon_buf"][want["recon"].size] ^= 1                            # the first byte behind it
        return got, want, "recon guard"
    if what == "container sentinel":
        r = want["mux_report"][-1]
        got["mux_buf"][int(r["out_offset"] + r["out_bytes"])] ^= 1
        return got, want, "container sentinel"
    assert what == "container moved"
    r = got["mux_report"][-1]
    o, nb = int(r["out_offset"]), int(r["out_bytes"])
    body = got["mux_buf"][o:o + nb].copy()
    got["mux_buf"][o:o + nb] = C.SENTINEL
    got["mux_buf"][o + 32:o + 32 + nb] = body
    got["mux_report"]["out_offset"][-1] = o + 32
    return got, want, "mux_report.out_offset"


altered.turn = 0


@pytest.mark.parametrize("what", ["time code", "record field", "recon inside", "recon outside", "container sentinel", "container moved"])
def test_the_checker_rejects_an_altered_expectation(what):
    for name, c in sorted(C.maximal().items()):
        C.check(C.render(c), C.expected(c), name)                               # the unaltered one passes
        for _ in range(3 if what == "record field" else 1):
            got, want, item = altered(c, what)
            with pytest.raises(C.Mismatch) as e:
                C.check(got, want, name)
            assert e.value.item == item and name in str(e.value), (what, e.value)
    # the mark of a stream byte says what it belongs to
    c = C.maximal()["cap"]
    got, want, _ = altered(c, "time code")
    with pytest.raises(C.Mismatch, match="time code of GOP"):
        C.check(got, want)


def test_zz_counts_and_time():
    """(last in the module: the figures of the docstring)"""
    print("tests/test_compose_cases.py: %d rows of pairs(), %d of port_pairs(), %d decoded streams, %.1f s so far"
          % (len(C.pairs()), len(C.port_pairs()), len(rows()), time.time() - T0))
