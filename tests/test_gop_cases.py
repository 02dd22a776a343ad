"""The premise and the reach of tests/gop_cases.py (no GPU): a stream spliced from the oracle's streams at several levels is a stream -
it decodes to the oracle's own reconstruction of every GOP at its level -, and the schedules and caps the -m gpu cases of
tests/test_gpu_gop_levels.py use reach every level, every number of tries and both sides of a GOP's exact size, so those byte
comparisons are not vacuous.  Plus the host side of the feature: the exports, the record's layout, the decoder's slice_qcodes."""
import ctypes
import os
import re

import numpy as np
import pytest

import gop_cases as G

M = G.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every clip with the GOP lengths the GPU cases use
USED = [("c64", 0), ("c80", 2), ("c96", 2), ("c96", 3)]


@pytest.mark.parametrize("name,pf", USED)
def test_headers_do_not_depend_on_the_level(name, pf):
    f, W, H = G.clip_args(name)
    heads = [G.cut(G.encoded(f, W, H, pf, q)[0])[0] for q in (1, 2, 3, 4)]
    assert len(heads[0]) == G.SEQ_HEADER_BYTES and heads[0] == heads[1] == heads[2] == heads[3]


@pytest.mark.parametrize("name,pf", USED)
def test_the_cut_finds_exactly_the_gops(name, pf):
    f, W, H = G.clip_args(name)
    for q in (1, 2, 3, 4):
        s = G.encoded(f, W, H, pf, q)[0]
        head, gops = G.cut(s)
        assert len(gops) == G.ngops(len(f), pf) == len(M.decoder.decode(s).gops)
        assert G.finish(head + b"".join(gops)) == s             # the end code and the padding follow the known rule
    sizes = G.gop_sizes(f, W, H, pf)
    assert all(sizes[q][k] > sizes[q + 1][k] for q in range(3) for k in range(len(sizes[0])))       # a coarser level is smaller, here


@pytest.mark.parametrize("name,pf", USED)
def test_spliced_stream_decodes_to_the_oracles_reconstruction(name, pf):
    f, W, H = G.clip_args(name)
    lv = G.per_gop(G.SCHEDULE, G.ngops(len(f), pf))
    s = G.splice(f, W, H, pf, G.SCHEDULE)
    d = M.decoder.decode(s, quirks=True)
    assert len(d.frames) == len(f)
    assert d.slice_qcodes == G.expected_qcodes(len(f), H, pf, G.SCHEDULE)
    y, c = W * H, W * H // 4
    for k in range(len(f)):
        rec = G.encoded(f, W, H, pf, lv[k // (pf + 1)])[1]["recon"][k]
        got = np.concatenate([p.reshape(-1) for p in d.frames[k]])
        assert got.size == y + 2 * c and np.array_equal(got, rec), (name, pf, k)
    # and it is not the stream of any single level
    assert all(s != G.encoded(f, W, H, pf, q)[0] for q in (1, 2, 3, 4))


def test_slice_qcodes_of_a_plain_stream():
    f, W, H = G.clip_args("c64")
    for q in (1, 2, 3, 4):
        d = M.decoder.decode(G.encoded(f, W, H, 0, q)[0])
        assert d.slice_qcodes == [[1 << q] * (H // 16)] * len(f)
        assert all("qcode" not in p and "slice_qcodes" not in p for p in d.pictures)


def test_the_checked_example():
    f, W, H = G.clip_args("c80")
    sizes = G.gop_sizes(f, W, H, 2)
    assert sizes == [[6049, 4775, 3479], [3552, 2654, 2031], [2261, 1581, 1274], [1424, 941, 782]]
    assert G.cap_levels(sizes, [1, 1, 1], 3500) == ([3, 2, 1], [3, 2, 1], [0, 0, 0])
    assert G.cap_levels(sizes, [1, 1, 1], 3552) == ([2, 2, 1], [2, 2, 1], [0, 0, 0])
    assert G.cap_levels(sizes, [1, 1, 1], 800) == ([4, 4, 4], [4, 4, 4], [1, 1, 0])


def test_the_search_stops_at_the_first_fit():
    """sizes that are not monotone in the level: "smallest" is the first fit going upwards"""
    sizes = [[100], [50], [120], [40]]
    assert G.cap_levels(sizes, [1], 60) == ([2], [2], [0])
    assert G.cap_levels(sizes, [3], 60) == ([4], [2], [0])
    assert G.cap_levels(sizes, [3], 30) == ([4], [2], [1])
    assert G.cap_levels(sizes, [4], 30) == ([4], [1], [1])


def test_what_the_cases_reach():
    cases = {k: G.cap_case(k) for k in G.CAP_CASES}
    rec = np.concatenate([c["records"] for c in cases.values()])
    assert set(rec["level"]) == {1, 2, 3, 4} and set(rec["tries"]) == {1, 2, 3, 4} and set(rec["over"]) == {0, 1}
    assert max(len(set(c["levels"])) for c in cases.values()) >= 3                      # three different levels in one sequence
    exact = cases["b3552"]["records"][0]
    assert exact["bytes"] == 3552 == cases["b3552"]["B"] and exact["level"] == 2 and exact["over"] == 0        # a cap equal to the size: stays
    assert cases["b3551"]["records"][0]["level"] == 3 and cases["b3551"]["records"][0]["tries"] == 3            # one byte less: goes up
    over = cases["b800"]["records"]
    assert list(over["over"]) == [1, 1, 0] and list(over["level"]) == [4, 4, 4] and (over["bytes"][:2] > 800).all()
    s = cases["sched"]
    assert s["levels"] != G.per_gop(s["sched"], 3) and any(a > b for a, b in zip(s["levels"], s["sched"]))      # the cap raises a schedule's start
    assert s["levels"][2] == s["sched"][2]
    assert list(cases["q4"]["records"]["tries"]) == [1] * 7 and cases["q4"]["records"]["over"].any()
    for c in cases.values():                                                             # every record: the size at the level reported
        sizes = G.gop_sizes(c["frames"], c["W"], c["H"], c["pf"])
        assert all(r["bytes"] == sizes[r["level"] - 1][r["gop"]] for r in c["records"])
        assert [len(g) for g in G.cut(c["stream"])[1]] == list(c["records"]["bytes"])
    # the schedules of the -m gpu cases: all four levels, three in one sequence
    assert len(set(G.SCHEDULE)) == 3 and {q for sc in (G.SCHEDULE, [1, 3], [4, 2, 1, 3, 2, 2]) for q in sc} == {1, 2, 3, 4}


def test_record_layout():
    assert ctypes.sizeof(M.GopStat) == 32 and M.GOP_STAT_DTYPE.itemsize == 32
    for name, _ in M.GopStat._fields_:
        assert getattr(M.GopStat, name).offset == M.GOP_STAT_DTYPE.fields[name][1], name
    txt = open(os.path.join(ROOT, "include", "m2v_mi355x.h")).read()
    body = re.search(r"typedef struct m2v_gop_stat \{(.*?)\} m2v_gop_stat;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in M.GopStat._fields_]


def test_library_exports_the_entries():
    L = M.lib()
    for name in ("m2v_set_gop_levels", "m2v_gop_report"):
        assert hasattr(L, name) and name in M.EXPORTS
    assert L.m2v_set_gop_levels(None, None, 0) == -1           # M2V_E_PARAM: no handle, no GPU needed
    assert L.m2v_gop_report(None, None, 0) == -1
    for name in ("set_gop_levels", "gop_report"):
        assert callable(getattr(M.Mpeg2Encoder, name))
    import inspect
    p = inspect.signature(M.Mpeg2Encoder.encode_tensor).parameters
    assert p["gop_levels"].default is None and p["gop_bytes_max"].default == 0
