"""CPU: the oracle alone puts every clip of tests/entropy_clips.py where tests/test_gpu_entropy.py needs it - every run/level code of
table B-14 in both banks of the look-up, every escape row and the clamps behind them, symbol lists that end at and run past the 64
symbols of a trip of pass 2, empty and full tiles, every coded block pattern, every DC differential in each of its four roles, every
vector delta with the wrap, a code at every bit offset of a word, slots exactly at the class boundaries.  All of it is computed by
entropy_clips.census, a numpy restatement of the symbol list k_mb builds, and the first test here - the anchor - is that the census's
code lengths add up to the oracle's mb_bits on every macroblock.  These are conditions on the generators as committed, asserted on
what the oracle produced and not on what a generator aimed at; nothing is left out of any of them but ten of the 3507 zero entries of the look-up, named in their test (the figures the tests print are
in the docstrings).  Every clip also goes through the clocked second reading of stages T/U/V and through the independent decoder.
numpy and the oracle only.

Wall time (measured once): 103 s for the 61 cases - about 25 s of it the clocked model and the decoder on the 4608 macroblocks of dc_roles and the 4736 of each inter_zeros clip,
11 s the six mutants - next to 425 s for the CPU suite without this module."""
import numpy as np
import pytest

import dense_clips as D
import entropy_clips as E
import m2v_load
from oracle import m2v_oracle_ctypes as orc
from test_rtl_stage_tuv import run_model

M = m2v_load.load()
CASES = E.cases()
T = E.tables()
PAIRS = [(r, s * a) for r, a in T["table_pairs"] for s in (1, -1)]                 # the 222 signed table codes


def levels(c, kind, intra, bank=None, extra=None):
    """the set of (run, level) of the symbols of a kind (E.TABLE / E.ESCAPE) in intra / non-intra macroblocks [of a bank]"""
    s = c["sym"]
    m = (s["kind"] == kind) & (s["intra"] == int(intra))
    if bank is not None:
        m &= s["bank"] == bank
    if extra is not None:
        m &= extra(s)
    return set(zip(s["run"][m].tolist(), s["level"][m].tolist()))


def union(kind_of_clip, fn):
    """fn(census) -> set, over the Q_LEVELs of a kind of clip: -> (the union, {Q: size of its set})"""
    got, per = set(), {}
    for kind, arg in CASES:
        if kind == kind_of_clip:
            g = fn(E.census_of(kind, arg))
            per[arg] = len(g)
            got |= g
    return got, per


# ---------------------------------------------------------------------------------------------------------------------------------
# the anchor
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=E.case_id)
def test_anchor_census_lengths_add_up_to_the_oracles_mb_bits_on_every_macroblock(case):
    """the census's code lengths = dense_clips.slot_bits, and with the dependent codes = the dump's mb_bits, on every macroblock"""
    c = E.census_of(*case)
    clip, pf, VL, Q = E.cached_clip(*case)
    assert c["nsym"].size > 0
    assert np.array_equal(c["slot_bits"], D.slot_bits(c["dump"], clip.shape[3] // 16, pf))
    assert np.array_equal(c["slot_bits"] + c["dep"], c["dump"]["mb_bits"].astype(np.int64))
    assert np.array_equal(c["seg"].sum(-1), c["slot_bits"]) and (c["p1"] >= 2).all() and (c["p1"] <= 6 + 2 * 11 + 20).all()


def test_anchor_on_seeded_content_with_mixed_intra_and_inter_macroblocks():
    """three synth.clips at VECTOR_LEVEL 1 - 3 and dense_clips.mix, I P P"""
    for VL in (1, 2, 3):
        for clip in (M.synth.clip(128, 64, 3, clip_index=VL, scene_len=2), D.mix(128, 64, 3, 5)):
            c = E.census(clip, 8, 4, 2, VL, VL)
            assert c["inter"][1:].any() and not c["inter"][1:].all()
            assert np.array_equal(c["slot_bits"], D.slot_bits(c["dump"], 8, 2))
            assert np.array_equal(c["slot_bits"] + c["dep"], c["dump"]["mb_bits"].astype(np.int64))


# ---------------------------------------------------------------------------------------------------------------------------------
# 1: table codes
# ---------------------------------------------------------------------------------------------------------------------------------
def test_1_every_table_code_in_intra_macroblocks_and_in_both_banks_of_non_intra_ones():
    """222 of 222 signed codes: as AC symbols of intra macroblocks (Q_LEVEL 1 / 2 / 3 / 4: 212 / 222 / 222 / 196 of them), behind
    another level of a non-intra block - bank 0 (218 / 222 / 222 / 190) - and, the 220 with a run >= 1 and (0, +-1) as the '1s' code,
    as the first symbol of a non-intra block - bank 1 (171 / 222 / 222 / 205), where the run is the zig-zag position; (0, +-1) also
    behind a level ('11s'); a first symbol at every position 0 .. 63"""
    intra, per = union("intra_codes", lambda c: levels(c, E.TABLE, True) & set(PAIRS))
    print("intra, per Q_LEVEL:", per)
    assert sorted(set(PAIRS) - intra) == []
    bank0, per = union("inter_codes", lambda c: levels(c, E.TABLE, False, 0) & set(PAIRS))
    print("non-intra bank 0, per Q_LEVEL:", per)
    assert sorted(set(PAIRS) - bank0) == []
    bank1, per = union("inter_codes", lambda c: levels(c, E.TABLE, False, 1) & set(PAIRS))
    print("non-intra bank 1, per Q_LEVEL:", per)
    assert sorted(set(PAIRS) - bank1) == []
    assert {(0, 1), (0, -1)} <= bank1 and {(0, 1), (0, -1)} <= bank0
    positions = set()
    for kind, arg in CASES:
        s = E.census_of(kind, arg)["sym"]
        b1 = (s["bank"] == 1) & (s["kind"] <= E.ESCAPE)
        assert np.array_equal(s["run"][b1], s["position"][b1]) and (s["intra"][b1] == 0).all()
        one = b1 & (s["run"] == 0) & (np.abs(s["level"]) == 1)
        assert (s["length"][one] == 2).all() and (s["length"][(s["kind"] == E.TABLE) & ~one] >= 3).all()
        positions |= set(s["position"][b1].tolist())
    assert positions == set(range(64))


# ---------------------------------------------------------------------------------------------------------------------------------
# 2: escapes
# ---------------------------------------------------------------------------------------------------------------------------------
def first_escapes(last_run):
    return {(r, s * (E.last_table_level(r) + 1)) for r in range(last_run + 1) for s in (1, -1)}


def test_2_the_first_escape_of_every_run_and_the_clamps_of_the_look_up():
    """intra: the first level without a table code at every run 0 .. 31 and +-1 at every run 32 .. 62, both signs - 126 of 126
    (Q_LEVEL 1 / 2 / 3 / 4: 123 / 126 / 126 / 124).  Non-intra: the same through run 63 as a block's first symbol - 128 of 128
    (110 / 128 / 128 / 126) - and through run 62 behind a level - 126 of 126 (120 / 126 / 126 / 124).  (0, +-40) with a table code,
    (0, +-41) and (0, +-42) escapes, and levels >= 41 at runs >= 32, intra and non-intra."""
    assert [E.last_table_level(r) for r in (0, 1, 2, 3, 6, 16, 31, 32)] == [40, 18, 5, 4, 3, 2, 1, 0]
    intra, per = union("intra_codes", lambda c: levels(c, E.ESCAPE, True) & first_escapes(62))
    print("intra, per Q_LEVEL:", per)
    assert sorted(first_escapes(62) - intra) == []
    first, per = union("inter_codes", lambda c: levels(c, E.ESCAPE, False, 1) & first_escapes(63))
    print("non-intra, a block's first symbol, per Q_LEVEL:", per)
    assert sorted(first_escapes(63) - first) == []
    behind, per = union("inter_codes", lambda c: levels(c, E.ESCAPE, False, 0) & first_escapes(62))
    print("non-intra, behind a level, per Q_LEVEL:", per)
    assert sorted(first_escapes(62) - behind) == []
    for kind, intra_mb in (("intra_codes", True), ("inter_codes", False)):
        tab, _ = union(kind, lambda c: levels(c, E.TABLE, intra_mb))
        esc, _ = union(kind, lambda c: levels(c, E.ESCAPE, intra_mb))
        assert {(0, 40), (0, -40)} <= tab
        assert {(0, 41), (0, -41), (0, 42), (0, -42)} <= esc
        both = sorted(e for e in esc if e[0] >= 32 and abs(e[1]) >= 41)
        print(kind, "levels >= 41 at runs >= 32:", both)
        assert len(both) >= 2 and {np.sign(v) for _, v in both} == {1, -1}


ZERO_MISSED_BANK0 = [(11, 30), (11, 35), (11, 37), (11, 40)]
ZERO_MISSED_BANK1 = [(3, 36), (5, 36), (21, 36), (23, 36), (25, 36), (27, 36)]


def test_2_every_entry_of_the_look_up_that_must_read_zero():
    """all 32 x 40 - 111 = 1169 (run, |level|) of the rows 0 .. 31 without a code, as escapes: 1169 of 1169 in intra macroblocks (Q_LEVEL 1 /
    2: 1090 / 1152); 1165 behind a level of a non-intra block (1108 / 1153) and 1163 as its first symbol (1028 / 1153) - the ten that
    the oracle's quantiser did not give back at either Q_LEVEL are named above, 0.3 % and 0.5 %, none of them the first escape of a row
    (those are the test before this one) - every row 15 .. 31 is complete in intra macroblocks and in bank 0"""
    want = {(r, abs(v)) for r, v in E.zero_targets()}
    assert len(want) == 1169

    def reached(kind, intra_mb, bank):
        def fn(c):
            s = c["sym"]
            m = (s["kind"] == E.ESCAPE) & (s["intra"] == int(intra_mb)) & ((s["bank"] == bank) | intra_mb)
            return set(zip(s["run"][m].tolist(), np.abs(s["level"][m]).tolist())) & want
        got, per = union(kind, fn)
        print(kind, "bank", bank, "per Q_LEVEL:", per)
        return got
    assert sorted(want - reached("intra_zeros", True, 0)) == []
    assert sorted(want - reached("inter_zeros", False, 0)) == ZERO_MISSED_BANK0
    assert sorted(want - reached("inter_zeros", False, 1)) == ZERO_MISSED_BANK1
    assert len(ZERO_MISSED_BANK0) + len(ZERO_MISSED_BANK1) <= 0.02 * 2 * len(want)
    assert not any(a == E.last_table_level(r) + 1 for r, a in ZERO_MISSED_BANK0 + ZERO_MISSED_BANK1)


def test_2_the_largest_escape_of_the_full_swing_basis_patterns():
    """test_gpu_extremes.basis_sign_frames at every Q_LEVEL (VECTOR_LEVEL 3, I + P): the escapes of largest magnitude of either sign
    that pixels produce, printed; entropy_clips.ESCAPE_EXTREMES holds them"""
    from test_gpu_extremes import basis_sign_frames
    got = {}
    for Q in E.Q_LEVELS:
        c = E.census(basis_sign_frames(128, 96, 10 * Q + 3), 8, 6, 1, 3, Q)
        s = c["sym"]
        lv = s["level"][s["kind"] == E.ESCAPE]
        got[Q] = (int(lv.min()), int(lv.max()))
        assert np.array_equal(c["slot_bits"], D.slot_bits(c["dump"], 8, 1))
    print("largest escapes (negative, positive) per Q_LEVEL:", got)
    assert got == E.ESCAPE_EXTREMES


# ---------------------------------------------------------------------------------------------------------------------------------
# 3: list indices
# ---------------------------------------------------------------------------------------------------------------------------------
LIST_ROOM = (1600 - 16) // 4                     # entries from s_sym to s_pred (csrc/m2v_kernels.hpp: lds + 16 .. kOffPred = kR1)


def counts_censuses():
    return [E.census_of("counts", Q) for Q in E.COUNTS_Q]


def test_3_symbol_counts_around_the_trips_of_pass_2_and_the_fullest_lists():
    """macroblocks of exactly 63, 64, 65, 127, 128 and 129 symbols, intra and non-intra, at Q_LEVEL 1 and 2 each; the fullest there
    are, every level +-1: 387 symbols intra (3 DC codes + 6 x (63 levels + end)) and 391 non-intra (pattern + 6 x (64 levels + end)),
    both the arithmetic maximum and both under the 396 entries the list has room for in front of s_pred"""
    for c in counts_censuses():
        for inter in (False, True):
            n = c["nsym"][c["inter"] == inter]
            assert {63, 64, 65, 127, 128, 129} <= set(n.tolist())
            print("largest list, %s: %d symbols" % ("non-intra" if inter else "intra", n.max()))
            assert n.max() == (391 if inter else 387) and n.max() <= LIST_ROOM


def test_3_segment_starts_and_every_kind_of_symbol_behind_the_first_trip():
    """idxB and idxC at 63, 64 and 65 each; a table code, an escape, a chained DC code and an end code at list indices >= 64; an escape
    AT an index that is a multiple of 64 (its run comes from the last symbol of the trip before), behind a level and behind a raw
    symbol (DC code, end code), intra and non-intra; an escape at an index >= 65 whose raw symbol in front sits at >= 64; and the '1s'
    code at index 64 and 128 (the bank comes from the last symbol of the trip before)"""
    for c in counts_censuses():
        intra = ~c["inter"]
        assert {63, 64, 65} <= set(c["idxB"][intra].tolist()) and {63, 64, 65} <= set(c["idxC"][intra].tolist())
        s = c["sym"]
        raw_front = np.isin(s["in_front"], (E.DC, E.PATTERN, E.END))
        for intra_mb in (1, 0):
            m = s["intra"] == intra_mb
            kinds = set(s["kind"][m & (s["index"] >= 64)].tolist())
            assert kinds >= ({E.TABLE, E.ESCAPE, E.DC, E.END} if intra_mb else {E.TABLE, E.ESCAPE, E.END})
            esc = m & (s["kind"] == E.ESCAPE)
            at = esc & (s["index"] % 64 == 0) & (s["index"] > 0)
            assert {64, 128} <= set(s["index"][at & raw_front].tolist()) and {64, 128} <= set(s["index"][at & ~raw_front].tolist())
            assert (esc & (s["index"] >= 65) & raw_front).any()
        one = (s["bank"] == 1) & (s["run"] == 0) & (np.abs(s["level"]) == 1) & (s["length"] == 2)
        assert {64, 128} <= set(s["index"][one].tolist())


# ---------------------------------------------------------------------------------------------------------------------------------
# 4: empty and full tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def test_4_empty_and_full_tiles():
    """an intra tile without an AC level as each of the six tiles, next to tiles that have some (as Y00 the macroblock's list starts
    with the end code); a tile whose last level sits at position 63; intra tiles with all 63 AC positions coded and non-intra tiles
    with all 64; a non-intra tile with a level at position 0, one at position 63 and nothing between"""
    for c in counts_censuses():
        coef, inter = c["dump"]["coef"].astype(np.int64), c["inter"]
        ac = (coef[..., 1:] != 0).sum(-1)                                   # [frames, mbs, 6]
        intra_with_ac = ~inter & (ac.sum(-1) > 0)
        for t in range(6):
            assert (intra_with_ac & (ac[..., t] == 0)).any(), t
        s = c["sym"]
        first = (s["index"] == 0) & (s["intra"] == 1)
        y00_empty = intra_with_ac & (ac[..., 0] == 0)
        assert (s["kind"][first & y00_empty[s["frame"], s["mb"]]] == E.END).all()
        assert (~inter & (ac.sum(-1) == 0)).any()                            # and a macroblock of nothing but DC
        assert (~inter[..., None] & (coef[..., 63] != 0) & (ac < 63)).any() and (inter[..., None] & (coef[..., 63] != 0)).any()
        assert (~inter[..., None] & (ac == 63)).any()
        assert (inter[..., None] & ((coef != 0).sum(-1) == 64)).any()
        only_ends = inter[..., None] & (coef[..., 0] != 0) & (coef[..., 63] != 0) & ((coef != 0).sum(-1) == 2)
        assert only_ends.any()


# ---------------------------------------------------------------------------------------------------------------------------------
# 5: coded block pattern, 9: macroblock types
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Q", E.PATTERNS_Q)
def test_5_every_pattern_first_in_a_slice_and_behind_an_inter_neighbour(Q):
    """64 of 64 patterns on inter macroblocks that are first in their slice, 64 of 64 behind an inter neighbour; pattern 0 with the
    zero vector and with another one; at Q_LEVEL 1 and 3 each"""
    c = E.census_of("patterns", Q)
    P = c["p_picture"] & c["inter"]
    assert set(c["cbp"][P & c["first"]].tolist()) == set(range(64))
    assert set(c["cbp"][P & c["left_inter"]].tolist()) == set(range(64))
    moving = (c["mv"] != 0).any(-1)
    assert (P & (c["cbp"] == 0) & moving).any() and (P & (c["cbp"] == 0) & ~moving).any()
    assert (c["nsym"][P & (c["cbp"] == 0)] == 0).all()


def test_9_every_macroblock_type_first_in_a_slice_and_behind_each_kind_of_neighbour():
    """P pictures: intra, inter with coefficients, inter without - each first in its slice, behind an intra and behind an inter one"""
    seen = set()
    for kind, arg in CASES:
        c = E.census_of(kind, arg)
        P = c["p_picture"]
        typ = np.where(~c["inter"], 0, np.where(c["cbp"] != 0, 1, 2))
        where = np.where(c["first"], 0, np.where(c["left_intra"], 1, 2))
        seen |= set(zip(typ[P].tolist(), where[P].tolist()))
        assert (c["p1"][P & (typ == 0)] >= 6 + 3).all() and (c["p1"][c["inter"]] >= 2 + 2).all()
    assert seen == {(t, w) for t in range(3) for w in range(3)}


# ---------------------------------------------------------------------------------------------------------------------------------
# 6: DC differentials
# ---------------------------------------------------------------------------------------------------------------------------------
def test_6_every_dc_differential_in_each_of_its_four_roles():
    """flat tiles of 0 .. 255 give DC levels -512 .. 508 in steps of 4 (the level is 4 (value - 128)); tiles one step from flat
    (entropy_clips.dc_tile) the levels between.  So a differential lies in -1020 .. 1020, and all 2041 values appear in the I picture
    of dc_roles in each role: Y00 against the left intra neighbour's Y11, Y01 / Y10 / Y11 chained, U, V - sizes 0 .. 10 of both signs.
    In the P picture Y00, U and V also start from 0 first in a slice and behind an inter neighbour, in P and I pictures."""
    lv = E.dc_levels(E.DC_Q)
    assert (lv.min(), lv.max()) == (-512, 508) and np.array_equal(lv, 4 * (np.arange(256) - 128))
    for Q in E.Q_LEVELS:
        assert np.array_equal(E.dc_levels(Q), lv)
    c = E.census_of("dc_roles", E.DC_Q)
    every = set(range(-1020, 1021))
    intra = ~c["inter"]
    neighbour = intra[0] & c["left_intra"][0]
    for name, at, tiles in (("Y00", neighbour, [0]), ("chained", intra[0], [1, 2, 3]), ("U", neighbour, [4]), ("V", neighbour, [5])):
        got = set(c["dcd"][0][at][:, tiles].reshape(-1).tolist())
        print("%s: %d of %d differentials" % (name, len(got & every), len(every)))
        assert got == every, name
    assert set(E.dc_size(np.array(sorted(every))).tolist()) == set(range(11))
    for pic in (0, 1):
        for at in (intra[pic] & c["first"][pic],) + ((intra[pic] & c["left_inter"][pic],) if pic else ()):
            assert at.sum() >= 8
            for t in (0, 4, 5):
                assert np.array_equal(c["dcd"][pic][at][:, t], c["dump"]["coef"][pic][at][:, t, 0]) and len(set(c["dcd"][pic][at][:, t].tolist())) >= 4


# ---------------------------------------------------------------------------------------------------------------------------------
# 7: vector deltas
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("VL", (1, 2, 3))
def test_7_every_vector_delta_and_every_vector_against_a_predictor_of_zero(VL):
    """mv - prev over -8 VL .. 8 VL on x and on y, all 17 / 33 / 49 values - for VECTOR_LEVEL 3 the 16 deltas that wrap (> 15, < -16),
    for 2 the one (16).  Every value -4 VL .. 4 VL against a predictor of 0 behind an intra neighbour, and first in a slice - there
    without mvx < 0, which the search masks at the frame's left border (search_clips.legal_vectors)"""
    R = 4 * VL
    assert R == max(abs(v) for xy in E.S.legal_vectors("interior", VL) for v in xy)
    c = E.census_of("deltas", VL)
    I = c["inter"]
    assert (c["pmv"][I & ~c["left_inter"]] == 0).all()
    for k in (0, 1):
        got = set(c["dmv"][I & c["left_inter"]][:, k].tolist())
        assert got == set(range(-2 * R, 2 * R + 1)), (k, sorted(set(range(-2 * R, 2 * R + 1)) - got))
        assert set(c["mv"][I & c["left_intra"]][:, k].tolist()) == set(range(-R, R + 1))
        assert set(c["mv"][I & c["first"]][:, k].tolist()) == set(range(0 if k == 0 else -R, R + 1))
    if VL == 3:
        d = c["dmv"][I & c["left_inter"]]
        assert (d > 15).sum() >= 16 and (d < -16).sum() >= 14


# ---------------------------------------------------------------------------------------------------------------------------------
# 8: bit positions
# ---------------------------------------------------------------------------------------------------------------------------------
def test_8_a_code_at_every_bit_offset_codes_that_end_on_and_straddle_a_word_and_slots_at_the_class_boundaries():
    """over the module's clips: a table code, an escape and a chained DC code start at each of the 32 bit offsets of a slot word; codes
    of every kind end exactly on a word boundary (lds_put's low half is 0) and straddle one; inside the slice image the three
    dependent codes and the three segments k_assemble places start at each of the 32 offsets too, end on boundaries and straddle
    them.  Slots of exactly 256, 257, 512, 513, 1024 and 1025 bits (and 255, 258, 511, 514, 1023, 1026), at Q_LEVEL 1 and 2."""
    starts = {k: set() for k in (E.TABLE, E.ESCAPE, E.DC)}
    ends, straddles = {k: 0 for k in range(5)}, {k: 0 for k in range(5)}
    dep = {k: [set(), 0, 0] for k in ("p1", "p2", "p3", "A", "B", "C")}
    for kind, arg in CASES:
        c = E.census_of(kind, arg)
        s = c["sym"]
        for k in range(5):
            m = s["kind"] == k
            if k in starts:
                starts[k] |= set((s["offset"][m] % 32).tolist())
            ends[k] += int(((s["offset"] + s["length"])[m] % 32 == 0).sum())
            straddles[k] += int((s["offset"][m] % 32 + s["length"][m] > 32).sum())
        parts = [("p1", c["at1"], c["p1"]), ("p2", c["at2"], c["p2"]), ("p3", c["at3"], c["p3"])] + \
                [(n, c["seg_at"][..., j], c["seg"][..., j]) for j, n in enumerate("ABC")]
        for name, at, ln in parts:
            at, ln = at[ln > 0], ln[ln > 0]
            dep[name][0] |= set((at % 32).tolist())
            dep[name][1] += int(((at + ln) % 32 == 0).sum())
            dep[name][2] += int((at % 32 + ln > 32).sum())
    print("codes that end on a word boundary:", {E.KINDS[k]: v for k, v in ends.items()}, "that straddle one:", {E.KINDS[k]: v for k, v in straddles.items()})
    for k in starts:
        assert starts[k] == set(range(32)), E.KINDS[k]
    for k in (E.TABLE, E.ESCAPE, E.DC, E.END):
        assert ends[k] > 0 and straddles[k] > 0, E.KINDS[k]
    for name, (offs, on, over) in dep.items():
        assert offs == set(range(32)) and on > 0 and over > 0, name
    for Q in E.SIZES_Q:
        c = E.census_of("sizes", Q)
        assert set(E.SIZE_BITS) <= set(c["slot_bits"].reshape(-1).tolist())
        assert np.array_equal(c["slot_bits"], D.slot_bits(c["dump"], E.SIZES_SHAPE[1], 0))


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle on the new ground: the clocked second reading of T / U / V, the independent decoder, the entropy mutants
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=E.case_id)
def test_the_clocked_model_and_the_decoder_agree_with_the_oracle(case):
    clip, pf, VL, Q = E.cached_clip(*case)
    c = E.census_of(*case)
    n, _, H, W = clip.shape
    assert run_model(W, H, Q, pf, c["dump"], n) == c["bytes"]
    out = M.decoder.decode(c["bytes"], quirks=True)
    assert (out.width, out.height) == (W, H) and len(out.frames) == n
    for f in range(n):
        assert np.array_equal(np.concatenate([p.reshape(-1) for p in out.frames[f]]), c["dump"]["recon"][f]), "frame %d" % f


ENTROPY_MUTANTS = (10, 11, 12, 14, 20, 21)
MUTANT_CASES = (("intra_codes", 4), ("inter_codes", 2), ("counts", 1), ("patterns", 1), ("deltas", 2))


def test_which_entropy_mutants_of_the_oracle_the_clips_expose_on_their_own():
    """the oracle compiled with one mis-reading of the entropy coder each (tests/test_oracle_mutants.py), on a sample of the clips,
    against the clocked model fed with the mutant's own decisions: 10 ('1s'), 11 (run 31), 12 (a zero first coefficient) and 21 (the
    wrap window of the vector delta) must be exposed; 14 and 20 (predictor resets) are reported.  Not part of the kill matrix."""
    clips = {case: E.cached_clip(*case) for case in MUTANT_CASES}              # built with the real oracle, before any switch
    paths = orc.build_mutants()
    exposed = {}
    for k in ENTROPY_MUTANTS:
        orc.use_library(paths[k])
        try:
            assert orc.lib().m2v_oracle_mutant() == k
            exposed[k] = []
            for case, (clip, pf, VL, Q) in clips.items():
                n, _, H, W = clip.shape
                data, d = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, dump=True)
                if run_model(W, H, Q, pf, d, n) != data:
                    exposed[k].append(E.case_id(case))
        finally:
            orc.use_library(None)
    for k in ENTROPY_MUTANTS:
        print("mutant %d exposed by: %s" % (k, ", ".join(exposed[k]) or "none of the sample"))
    assert all(exposed[k] for k in (10, 11, 12, 21)), exposed
