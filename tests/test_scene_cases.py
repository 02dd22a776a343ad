"""The premise and the reach of tests/scene_cases.py (no GPU): a stream spliced from the oracle's streams of every GOP encoded alone,
with the time code patched, is the stream - with no forced start it IS the oracle's whole stream -, it decodes to picture types,
temporal references and frames per the layout, and T = 3000 separates the clips' scene changes from everything else.  Plus the host
side of the feature: m2v_gop_layout against the rule in plain Python, the exports, the record's layout."""
import ctypes
import os
import random
import re

import numpy as np
import pytest

import gop_cases as G
import scene_cases as S

M = G.M
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE_LEN = {k: v["scene_len"] for k, v in G.CLIPS.items()}


@pytest.mark.parametrize("name", ["c64", "c80", "c96"])
@pytest.mark.parametrize("pf", [0, 2, 3])
def test_no_forced_start_is_the_oracles_whole_stream(name, pf):
    """this pins the time-code patch: every GOP of the whole stream is GOP 0 of its frames alone, but for the time code"""
    f, W, H = G.clip_args(name)
    assert S.expected(f, W, H, pf, None) == G.encoded(f, W, H, pf, 2)[0]
    assert S.expected(f, W, H, pf, [0, pf + 1, 1000]) == G.encoded(f, W, H, pf, 2)[0]


def test_time_code():
    assert S.time_code(0) == bytes([0x00, 0x08, 0x00, 0x40])
    assert S.time_code(23) == bytes([0x00, 0x08, 0x0B, 0xC0])
    assert S.time_code(24) == bytes([0x00, 0x08, 0x20, 0x40])
    assert S.time_code(1440)[:2] == bytes([0x00, 0x18])
    assert S.time_code(86400 * 70)[0] >> 2 == 63


@pytest.mark.parametrize("name,pf,starts", [("c96", 3, [5]), ("c96", 255, [1, 2, 3]), ("c64", 0, [2, 4]), ("c80", 2, [0, 3, 6, 100])])
def test_expected_stream_decodes_per_layout(name, pf, starts):
    f, W, H = G.clip_args(name)
    s = S.expected(f, W, H, pf, starts)
    d = M.decoder.decode(s, quirks=True)
    fl = S.layout(len(f), pf, starts)
    gs = S.gops(len(f), pf, starts)
    assert len(d.frames) == len(f) and len(d.gops) == len(gs)
    assert [p["type"] for p in d.pictures] == [1 if x else 2 for x in fl]
    assert [p["temporal_reference"] for p in d.pictures] == [k for _, L in gs for k in range(L)]
    at = 0
    for a, L in gs:
        alone = M.decoder.decode(G.encoded(f[a:a + L], W, H, pf, 2)[0], quirks=True)
        for k in range(L):
            for p, q in zip(d.frames[at + k], alone.frames[k]):
                assert np.array_equal(p, q), (name, a, k)
        at += L


def test_layout_examples():
    assert S.gops(12, 3, [5]) == [(0, 4), (4, 1), (5, 4), (9, 3)]
    assert S.layout(12, 3, [5]) == [1, 0, 0, 0, 2, 4, 0, 0, 0, 2, 0, 0]
    assert S.gops(12, 255, [1, 2, 3]) == [(0, 1), (1, 1), (2, 1), (3, 9)]
    assert S.layout(8, 2, [0, 3, 6, 100]) == [5, 0, 0, 6, 0, 0, 6, 0]
    assert S.layout(12, 3, [5], cuts=[4, 8]) == [1, 0, 0, 0, 10, 4, 0, 0, 8, 0, 0, 0]


def test_gop_layout_equals_the_rule():
    rng = random.Random(1234)
    for trial in range(200):
        pf = rng.choice([0, 255, 1, 2, 3, 7, rng.randrange(256)]) if trial > 3 else (0, 255, 0, 255)[trial]
        nf = rng.randrange(0, 80) if trial % 7 else rng.randrange(250, 600)
        pool = list(range(nf + 10))
        starts = sorted(rng.sample(pool, rng.randrange(0, min(len(pool), 12) + 1)))
        if trial % 3 == 0 and nf:
            starts = sorted(set(starts) | {0, min(pf + 1, nf + 5), nf + 3})       # 0, a cadence position, one past the end
        want = S.layout(nf, pf, starts)
        flags, n = M.gop_layout(pf, starts, nf)
        assert flags.tolist() == want and n == sum(1 for x in want if x), (pf, starts, nf)
    assert M.gop_layout(3, None, 9)[1] == 3 and M.gop_layout(3, [], 0)[1] == 0
    assert M.gop_layout(256 + 3, [5], 12)[0].tolist() == S.layout(12, 3, [5])       # pframes_count & 0xFF
    L = M.lib()
    bad = (ctypes.c_uint32 * 3)(4, 4, 9)
    assert L.m2v_gop_layout(3, bad, 3, 12, None) == -1
    bad = (ctypes.c_uint32 * 2)(9, 4)
    assert L.m2v_gop_layout(3, bad, 2, 12, None) == -1
    with pytest.raises(ValueError):
        M.gop_layout(3, [9, 4], 12)


@pytest.mark.parametrize("name,smallest_at,largest_else", [("c64", 5698, 2071), ("c80", 4084, 1747), ("c96", 5555, 1576)])
def test_threshold_3000_separates_the_scene_changes(name, smallest_at, largest_else):
    f, W, H = G.clip_args(name)
    mbs = (W // 16) * (H // 16)
    d = S.diffs(f)
    sl = SCENE_LEN[name]
    at = [int(d[n]) // mbs for n in range(1, len(f)) if n % sl == 0]
    other = [int(d[n]) // mbs for n in range(1, len(f)) if n % sl]
    print(name, "D/mbs at scene changes", at, "elsewhere", other)
    assert min(at) == smallest_at and max(other) == largest_else
    assert d[0] == 0
    assert S.cuts_of(f, 3000) == [n for n in range(1, len(f)) if n % sl == 0]


def test_mb_sums_by_hand():
    f = np.zeros((2, 3, 32, 48), np.uint8)
    f[1, 0, 16:, 32:] = 255
    f[1, 0, 0, 0] = 7
    f[1, 1:] = 99                                       # chroma does not count
    s = S.mb_sums(f)
    assert s.shape == (2, 2, 3) and s[1].tolist() == [[7, 0, 0], [0, 0, 65280]] and S.diffs(f).tolist() == [0, 65287]


def test_record_layout():
    assert ctypes.sizeof(M.SceneStat) == 16 and M.SCENE_STAT_DTYPE.itemsize == 16
    for name, _ in M.SceneStat._fields_:
        assert getattr(M.SceneStat, name).offset == M.SCENE_STAT_DTYPE.fields[name][1], name
    txt = open(os.path.join(ROOT, "include", "m2v_mi355x.h")).read()
    body = re.search(r"typedef struct m2v_scene_stat \{(.*?)\} m2v_scene_stat;", txt, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [n for decl in body.split(";") for n in re.findall(r"(\w+)\s*(?:,|$)", decl.strip())]
    assert names == [n for n, _ in M.SceneStat._fields_]
    assert re.search(r"M2V_GOP_FIRST = 1, M2V_GOP_CADENCE = 2, M2V_GOP_LIST = 4, M2V_GOP_CUT = 8", txt)
    assert (M.GOP_FIRST, M.GOP_CADENCE, M.GOP_LIST, M.GOP_CUT) == (S.FIRST, S.CADENCE, S.LIST, S.CUT) == (1, 2, 4, 8)


def test_library_exports_the_entries():
    L = M.lib()
    for name in ("m2v_set_gop_starts", "m2v_gop_layout", "m2v_scene_report"):
        assert hasattr(L, name) and name in M.EXPORTS
    assert L.m2v_set_gop_starts(None, None, 0) == -1            # M2V_E_PARAM: no handle, no GPU needed
    assert L.m2v_scene_report(None, None, 0) == -1
    for name in ("set_gop_starts", "scene_report"):
        assert callable(getattr(M.Mpeg2Encoder, name))
    import inspect
    p = inspect.signature(M.Mpeg2Encoder.encode_tensor).parameters
    assert p["gop_starts"].default is None and p["scene_cut"].default == 0
