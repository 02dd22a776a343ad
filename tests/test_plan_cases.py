"""The streams of tests/plan_cases.py on the CPU: the g++ host build of every option's functions (tools/dec_*_host.hpp, a serial plan)
gives what decoder.decode gives - frames, counts, verdict, err_offset; the partition model; what every stream reaches, as literals;
the content rule; and for every quantity a plan carries from range to range a twin stream in which only that quantity's source
differs, whose frames change exactly where they must.  tests/test_gpu_decode_plan.py runs the same streams through the plan kernels."""
import numpy as np
import pytest

import plan_cases as P

D, M = P.D, P.M

# name -> (start codes, per, pictures, what plan_cases.reached lists)
REACH = {
    "edge_255": (255, 1, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor transparent_only empty_lanes"),
    "edge_256": (256, 1, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor transparent_only"),
    "edge_257": (257, 2, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor transparent_only empty_lanes"),
    "edge_511": (511, 2, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor transparent_only"),
    "edge_512": (512, 2, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice next_anchor_two_ranges_behind last_anchor transparent_only"),
    "edge_513": (513, 3, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice next_anchor_two_ranges_behind last_anchor transparent_only empty_lanes"),
    "edge_767": (767, 3, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_extension_slice next_anchor_two_ranges_behind last_anchor transparent_only"),
    "edge_769": (769, 4, 4,
        "anchors_0 anchors_1 one_anchor_behind_none b_anchors_in_two_earlier_ranges p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor transparent_only empty_lanes"),
    "shift_0": (1702, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_0_interlaced": (1662, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_1": (1714, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_1_interlaced": (1671, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_2": (1726, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_2_interlaced": (1680, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_3": (1738, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_3_interlaced": (1689, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_4": (1750, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_4_interlaced": (1698, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_5": (1762, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_5_interlaced": (1707, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_6": (1774, 7, 540,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "shift_6_interlaced": (1716, 7, 400,
        "anchors_0 anchors_1 anchors_2 one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "long_b": (3093, 13, 1000,
        "anchors_1 anchors_2 anchors_3_or_more b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
    "long_x": (2071, 9, 520,
        "anchors_0 anchors_1 anchors_2 anchors_3_or_more one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor load_used_two_ranges_behind sequence_then_load load_then_sequence empty_lanes more_than_256_pictures"),
    "long_t": (2071, 9, 520,
        "anchors_0 anchors_1 anchors_2 anchors_3_or_more one_anchor_behind_none b_anchors_in_two_earlier_ranges b_anchors_in_one_earlier_range b_anchor_in_own_range p_reference_first_of_range p_reference_two_ranges_back i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_slice_slice cut_gop_picture next_anchor_two_ranges_behind last_anchor load_used_two_ranges_behind sequence_then_load load_then_sequence empty_lanes more_than_256_pictures"),
    "long_m": (1548, 7, 470,
        "anchors_0 anchors_1 anchors_2 anchors_3_or_more p_reference_first_of_range i_last_of_range i_first_of_range cut_header_extension cut_extension_slice cut_gop_picture last_anchor empty_lanes event_list_regrown more_than_256_pictures"),
}
ALTERED_REFUSED = 88                                               # of 120: between 20 % and 90 %


def types_of(letters):
    return [" IPB".index(c) for c in letters]


def hold(stream, opt, layout="i420"):
    """the host build against the definition -> the definition's answer"""
    d, at = P.spec_cached(stream, opt)
    got, r = P.host_decode(stream, opt, layout)
    if d is None:
        assert got is None and (r["status"], r["err_offset"]) == (D.SYNTAX, at), (r, at)
        return None
    assert got is not None, r
    want = D.frames_of(d, layout)
    assert got.shape == want.shape and np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0][:8]
    rec = P.record_of(d, stream)
    assert {k: int(r[k]) for k in rec} == rec
    return d


def test_partition_model():
    """ranges(nev): 256 ranges of per events that cover [0, nev) in order, the trailing ones empty"""
    for nev in (0, 1, 255, 256, 257, 511, 512, 513, 767, 769, 1702, 3093):
        r = P.ranges(nev)
        per = P.per_of(nev)
        assert len(r) == 256 and r[0][0] == 0 and r[-1][1] == nev and all(a[1] == b[0] for a, b in zip(r, r[1:]))
        assert all(b - a == per for a, b in r if b < nev) and all(0 <= b - a <= per for a, b in r)
    assert [b - a for a, b in P.ranges(257)] == [2] * 128 + [1] + [0] * 127
    assert P.per_of(256) == 1 and P.per_of(257) == 2 and P.per_of(512) == 2 and P.per_of(513) == 3 and P.per_of(769) == 4


def test_order_model():
    """display_of and refs_of against the definition's display order, on every case's picture types"""
    for name, (s, L, opt, letters) in P.cases().items():
        t = types_of(letters)
        assert P.display_of(t) == M.decoder.display_order(t), name
        assert sorted(P.display_of(t)) == list(range(len(t)))


@pytest.mark.parametrize("name", sorted(REACH))
def test_case(name):
    """the host build gives the definition's frames, counts and verdict; the stream holds what REACH says, and keeps the content rule"""
    s, L, opt, letters = P.cases()[name]
    d = hold(s, opt)
    assert d is not None and [p["type"] for p in d.pictures] == types_of(letters)
    lay = P.layout_of(s)
    assert (lay["nev"], lay["per"], len(lay["pictures"]), " ".join(P.reached(s))) == REACH[name]
    assert lay["nev"] == len(M.decoder.start_codes(s)) == d.units
    assert P.content_faults(D.frames_of(d), types_of(letters)) == []


def test_reach_is_complete():
    """every crossing is held by some case; per goes from 1 to 13"""
    union = set()
    for name, (nev, per, npics, held) in REACH.items():
        union |= set(held.split())
    assert union == set(P.CROSSINGS)
    assert {v[1] for v in REACH.values()} >= {1, 2, 3, 4, 7, 9, 13}
    assert sorted(REACH) == sorted(P.cases())


def test_edges_are_exact():
    for n in P.EDGES:
        s = P.cases()["edge_%d" % n][0]
        assert len(M.decoder.start_codes(s)) == n
    assert [b - a for a, b in P.ranges(257)][128:130] == [1, 0]


def test_shift():
    """the same frames for every k, the same per, another es_bytes; every position of a picture's units meets a range's edge"""
    for tail, opt in (("", P.B_), ("_interlaced", P.BI)):
        want = D.frames_of(P.spec_cached(P.cases()["shift_0" + tail][0], opt)[0])
        sizes, firsts = set(), set()
        for k in range(P.SHIFT_PER):
            s, L, o, letters = P.cases()["shift_%d%s" % (k, tail)]
            assert o == opt and np.array_equal(D.frames_of(P.spec_cached(s, opt)[0]), want), k
            lay = P.layout_of(s)
            assert lay["per"] == P.SHIFT_PER
            sizes.add(len(s))
            starts = [a for a, b in P.ranges(lay["nev"]) if 0 < a < b]
            firsts |= {"picture" if lay["kinds"][a] in ("pic1", "pic2", "pic3") else lay["kinds"][a] for a in starts}
            firsts |= {"second slice" for a in starts if lay["kinds"][a - 1] == lay["kinds"][a] == "slice"}
        assert len(sizes) == P.SHIFT_PER
        assert firsts >= {"picture", "pic_ext", "slice", "gop", "seq", "seq_ext", "display", "skip"} | ({"second slice"} if tail else set()), firsts


def test_long_b_under_later_options():
    """long_b is accepted by every later option set; long_m, long_x and long_t by theirs"""
    s = P.cases()["long_b"][0]
    for opt in P.later_options(P.B_):
        assert hold(s, opt) is not None, opt
    assert [P.PLAN_OF[o] for o in [P.B_] + P.later_options(P.B_)] == ["k_db_plan", "k_di_plan", "k_dx_plan", "k_dt_plan"]
    assert hold(s, P.M_) is None
    assert hold(P.cases()["long_m"][0], P.B_) is not None


# ---- sensitivity ----
def changed(a, b):
    assert a.shape == b.shape
    return {int(d) for d in np.nonzero((a != b).any(axis=1))[0]}


@pytest.mark.parametrize("kind", ("anchor", "swap"))
def test_twin_of_shift(kind):
    """one anchor's level changed: it, the B pictures that read it and the chain of P pictures behind it change, nothing else - the last
    two anchors and the slot a picture is shown in are what is carried; two adjacent B pictures exchanged: their two display slots"""
    s, twin, want, src, letters = P.shift_twin(kind)
    a, b = P.host_decode(s, P.B_)[0], P.host_decode(twin, P.B_)[0]
    assert hold(twin, P.B_) is not None
    assert changed(a, b) == want and len(want) >= 2
    lay, disp = P.layout_of(s), P.display_of(types_of(letters))
    lanes = {lay["pictures"][disp.index(d)]["lane"] for d in want}
    assert max(lanes) > lay["pictures"][src]["lane"]


@pytest.mark.parametrize("kind", ("load", "reset"))
def test_twin_of_long_x(kind):
    """one quant_matrix_extension removed, one repeated sequence header removed: the pictures whose matrix in force is another one
    and what predicts from them change, nothing else"""
    s, twin, want, gone, letters = P.matrix_twin(kind)
    a, b = P.host_decode(s, P.XB)[0], P.host_decode(twin, P.XB)[0]
    assert hold(twin, P.XB) is not None
    disp = P.display_of(types_of(letters))
    assert changed(a, b) == {disp[p] for p in want} and len(want) >= 3
    lay = P.layout_of(s)
    assert max(lay["pictures"][p]["lane"] for p in want) > lay["pictures"][gone]["lane"]


# ---- refusals ----
REFUSED_AT = dict(i_far_b=3070, i_far_p_far_b=None, two_faults=12896, later_fault_alone=23271, b_option_off=134, extension_missing_at_range_end=2249,
                  gap_behind_first_chunk=19521)


def test_refusals():
    """the offset stated by hand (from the writer's log, and here as a number), the definition's and the host build's"""
    r = P.refusals()
    assert sorted(r) == sorted(REFUSED_AT)
    for name, (s, opt, at) in sorted(r.items()):
        assert at == REFUSED_AT[name], name
        d = hold(s, opt)
        assert (d is None) == (at is not None) and P.spec_cached(s, opt)[1] == at, name
    # the B picture of i_far_b lies several ranges behind its only anchor; the two faults lie about 1 000 events apart
    lay = P.layout_of(r["i_far_b"][0])
    assert lay["per"] >= 2 and lay["pictures"][1]["lane"] - lay["pictures"][0]["lane"] >= 3
    lay = P.layout_of(r["two_faults"][0])
    lo, hi = (lay["offsets"].index(REFUSED_AT[k]) for k in ("two_faults", "later_fault_alone"))
    assert 900 <= hi - lo <= 1200 and r["two_faults"][0][REFUSED_AT["later_fault_alone"] + 3] == 2
    s = r["extension_missing_at_range_end"][0]
    lay = P.layout_of(s)
    i = lay["offsets"].index(REFUSED_AT["extension_missing_at_range_end"])
    assert lay["kinds"][i] == "slice" and lay["kinds"][i - 1].startswith("pic") and i % lay["per"] == 0
    lay = P.layout_of(r["gap_behind_first_chunk"][0])
    assert sum(k.startswith("pic") and k != "pic_ext" for k in lay["kinds"][:lay["offsets"].index(REFUSED_AT["gap_behind_first_chunk"])]) > 256


def test_altered():
    """120 alterations of a 600-event stream: the host build gives the definition's verdict, offset and frames; the share refused"""
    s, L, letters = P.altered_base()
    lay = P.layout_of(s)
    assert lay["per"] == 3 and 550 <= lay["nev"] <= 650 and 140 <= len(lay["pictures"]) <= 200
    cases = P.altered()
    assert len(cases) == 120 and len({x for _, x in cases}) >= 110
    refused = sum(hold(x, P.B_) is None for _, x in cases)
    assert refused == ALTERED_REFUSED and 24 <= refused <= 108
