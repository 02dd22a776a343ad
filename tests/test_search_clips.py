"""CPU: the oracle alone puts every clip of tests/search_clips.py where tests/test_gpu_search.py needs it - every legal vector chosen,
in the interior and on every edge and corner; every full-pel candidate in a tie that only the scan order decides; every pair of
half-pel positions tied at the minimum; the intra cost tied with the best half-pel SAD, and one unit to either side; border macroblocks
whose match lies on masked candidates.  All of it is computed by search_clips.census, a numpy restatement of the oracle's
motion_stage, and the first test here is that the census reproduces the oracle's decision and vector on every macroblock of every
clip.  These are conditions on the generators as committed: a retuned generator that misses one fails here, on the CPU, instead of
leaving a GPU test that no longer reaches its corner.  numpy and the oracle only.

Wall time (measured once, one core): 82 s for the 283 cases, most of it building the edge and corner clips of VECTOR_LEVEL 2 and 3
(hundreds of GOPs, each built against the oracle's reconstruction); the CPU suite was 270 s without this module."""
import itertools

import numpy as np
import pytest

import m2v_load
import search_clips as S

M = m2v_load.load()
CASES = S.cases()


@pytest.mark.parametrize("conformant", [False, True])
@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_census_equals_the_oracle_on_every_macroblock(case, conformant):
    """decision and vector, both roundings of the four-sample mean; every VECTOR_LEVEL is among the cases"""
    c = S.census_of(*case, conformant=conformant)
    assert c["inter"].size > 0
    assert S.census_equals_oracle(c) == []


def test_census_equals_the_oracle_on_seeded_content_with_intra_macroblocks():
    """the clips above are nearly all inter: synth.clip with a scene cut and strong noise (every candidate dead: intra) as well"""
    rng = np.random.default_rng(5)
    for VL in S.VECTOR_LEVELS:
        for clip in (M.synth.clip(160, 96, 6, clip_index=3, scene_len=3), rng.integers(0, 256, (3, 3, 96, 160), dtype=np.uint8),
                     (128 + rng.integers(-40, 41, (3, 3, 96, 160))).astype(np.uint8)):
            c = S.census(clip, 10, 6, 2, VL, 2)
            assert S.census_equals_oracle(c) == []


def chosen(c, at):
    """the (mvx, mvy) of the inter macroblocks among `at` [mbh, mbw] bool, all pictures"""
    o = c["oracle"]
    inter = (o["mb_inter"] != 0) & at
    return set(zip(o["mb_mvx"][inter].tolist(), o["mb_mvy"][inter].tolist()))


@pytest.mark.parametrize("seed", S.INTERIOR_SEEDS)
@pytest.mark.parametrize("Q", S.Q_LEVELS)
@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_all_vectors_interior_every_vector_is_chosen(VL, Q, seed):
    """all 81 / 289 / 625, in each of the two P pictures, by the macroblock it was assigned to; no assigned macroblock intra"""
    c = S.census_of("interior", VL, Q, (seed,))
    _, maps, mask = S.all_vectors_built(VL, Q, seed, "interior")
    o = c["oracle"]
    assert mask.sum() == (8 * VL + 1) ** 2
    assert (o["mb_inter"][:, mask] != 0).all()
    assert np.array_equal(o["mb_mvx"][:, mask], maps[:, mask, 0]) and np.array_equal(o["mb_mvy"][:, mask], maps[:, mask, 1])
    for p in range(2):
        assert chosen({"oracle": {k: v[p:p + 1] for k, v in o.items()}}, mask) == set(S.legal_vectors("interior", VL))


@pytest.mark.parametrize("Q", S.Q_LEVELS)
@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_all_vectors_edges_and_corners_every_legal_vector_is_chosen(VL, Q):
    """(4 VL + 1)(8 VL + 1) vectors on each edge, (4 VL + 1)^2 in each corner"""
    c = S.census_of("border", VL, Q, (0,))
    for k in S.KLASSES[1:]:
        legal = set(S.legal_vectors(k, VL))
        assert len(legal) == (4 * VL + 1) * ((8 * VL + 1) if k in ("top", "bottom", "left", "right") else (4 * VL + 1))
        got = chosen(c, c["klass"] == S.KLASSES.index(k))
        assert got == legal, (k, sorted(legal - got), sorted(got - legal))


@pytest.mark.parametrize("case", CASES, ids=S.case_id)
def test_no_macroblock_carries_a_vector_its_position_masks(case):
    c = S.census_of(*case)
    for k in S.KLASSES:
        got = chosen(c, c["klass"] == S.KLASSES.index(k))
        assert got <= set(S.legal_vectors(k, case[1])), (k, sorted(got - set(S.legal_vectors(k, case[1]))))


def ties_censuses(VL):
    return [S.census_of("ties", VL, Q, (seed,)) for Q in S.Q_LEVELS for seed in S.TIES_SEEDS]


def tied_pairs(c):
    """the (dy, dx) pairs (scan order) of the partial full-pel ties of a census, as two [n, 2] arrays"""
    first, second = [], []
    for members in c["tie"][S.partial_ties(c)]:
        idx = np.flatnonzero(members)
        i, j = np.triu_indices(len(idx), 1)
        first.append(c["cand"][idx[i]])
        second.append(c["cand"][idx[j]])
    return np.concatenate(first), np.concatenate(second)


@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_ties_every_full_pel_candidate_is_in_a_partial_tie(VL):
    """a tie set of at least 2 members and fewer than all live candidates: the scan order decides, and a kernel that orders one pair
    of candidates the wrong way chooses another vector.  Also the relations between two tied candidates: the same dy, the same dx,
    and dy1 < dy2 with dx1 > dx2 - the one that tells a dy-major order from a dx-major one."""
    members = sum(c["tie"][S.partial_ties(c)].sum(0) for c in ties_censuses(VL))
    winners = set()
    rel = np.zeros(3, np.int64)
    for c in ties_censuses(VL):
        pt = S.partial_ties(c)
        winners |= set(zip(c["fy"][pt].tolist(), c["fx"][pt].tolist()))
        a, b = tied_pairs(c)
        rel += [(a[:, 0] == b[:, 0]).sum(), (a[:, 1] == b[:, 1]).sum(), ((a[:, 0] < b[:, 0]) & (a[:, 1] > b[:, 1])).sum()]
    print("VECTOR_LEVEL %d: %d partial ties; every candidate a member of at least %d; %d of %d candidates won one; tied pairs with the same dy %d,"
          " the same dx %d, dy1 < dy2 and dx1 > dx2 %d" % (VL, sum(int(S.partial_ties(c).sum()) for c in ties_censuses(VL)), members.min(),
                                                           len(winners), len(members), *rel))
    assert len(members) == (4 * VL + 1) ** 2 and (members >= 1).all(), np.flatnonzero(members == 0)
    assert (rel >= 1).all(), rel


@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_ties_every_pair_of_half_pel_positions_ties_at_the_minimum(VL):
    """all 36 pairs of the nine positions; the pairs the masks exclude are computed (those never unmasked together in any
    macroblock of the clips: none, the clips have interior macroblocks whose full-pel vector is inside the range)"""
    count, possible = {}, set()
    for c in ties_censuses(VL):
        for k, v in S.half_pel_ties(c).items():
            count[k] = count.get(k, 0) + v
        unmasked = c["v10"][..., :9].reshape(-1, 9) != 4096
        possible |= {(a, b) for a, b in itertools.combinations(range(9), 2) if (unmasked[:, a] & unmasked[:, b]).any()}
    print("VECTOR_LEVEL %d: macroblocks in which the pair ties at the minimum: %s" % (VL, " ".join("%d%d:%d" % (a, b, n) for (a, b), n in sorted(count.items()))))
    assert len(possible) == 36
    assert [k for k in sorted(possible) if count[k] == 0] == []


@pytest.mark.parametrize("i", S.INTRA_TIE_POSITIONS)
@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_intra_tie_is_a_tie_and_its_neighbours_decide_the_other_way(VL, i):
    """v10[9] == v10[i] == min(v10) == 4095: position 8 beats the intra cost, the intra cost beats every other position
    (find_min_in_10_values: 8, 9, 4, 5, 6, 7, 0 - 3).  One unit less at position i and it wins; one more (the 13th bit) and it is out."""
    by, bx = S.BUILT_BY, S.BUILT_BX
    mv = (i % 3 - 1, i // 3 - 1)
    want = {-1: (1,) + mv, 0: (1,) + mv if i == 8 else (0, 0, 0), 1: (0, 0, 0)}
    for off in (-1, 0, 1):
        c = S.census_of("intra_tie", VL, S.BUILT_Q, (i, off))
        v10, o = c["v10"][0, by, bx], c["oracle"]
        if off == 0:
            assert v10[9] == v10[i] == v10.min() == 4095 and (v10 == 4095).sum() == 2
        else:
            assert v10[9] == 4095 and (v10[i] == 4094 if off < 0 else v10[i] >= 4096) and np.delete(v10, [i, 9]).min() > 4095
        assert (int(o["mb_inter"][0, by, bx]), int(o["mb_mvx"][0, by, bx]), int(o["mb_mvy"][0, by, bx])) == want[off], (off, v10)


@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_outward_border_macroblocks_stay_inside_and_still_move(VL):
    """pictures 0 .. 3: the match lies beyond the left, right, top, bottom border.  No macroblock of that border carries a component
    through it (the general condition is test_no_macroblock_carries_a_vector_its_position_masks); at least one per side is inter with
    a non-zero vector all the same, inward or along the border"""
    for Q in S.Q_LEVELS:
        c = S.census_of("outward", VL, Q)
        o = c["oracle"]
        inter, mvx, mvy = o["mb_inter"] != 0, o["mb_mvx"], o["mb_mvy"]
        sides = ((np.s_[0, :, 0], mvx, 1), (np.s_[1, :, -1], mvx, -1), (np.s_[2, 0, :], mvy, 1), (np.s_[3, -1, :], mvy, -1))
        for at, comp, inward in sides:
            assert (comp[at][inter[at]] * inward >= 0).all()
            assert (inter[at] & ((mvx[at] != 0) | (mvy[at] != 0))).any()
        # and away from that border the search runs into the end of its range: the match is farther than it reaches
        assert (mvx[0, :, 1:] == -4 * VL).mean() > 0.5 and (mvy[3, :-1] == 4 * VL).mean() > 0.5


@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_interior_clips_carry_every_vertical_component_across_the_strip_boundaries(VL):
    """tests/test_gpu_search.py cuts the interior clips into 2 and 3 strips of macroblock rows.  Over the seeds used, the last row of
    a strip holds inter macroblocks with every mvy in 1 .. 4 VL (they read the strip below) and the first row of a strip every mvy in
    -4 VL .. -1 (the strip above)"""
    down, up = set(), set()
    for world in (2, 3):
        rows = M.parallel.partition_rows(8 * VL + 3, world)
        for seed in S.INTERIOR_SEEDS:
            d, u = S.vectors_crossing(S.census_of("interior", VL, 1, (seed,)), rows)
            down |= d
            up |= u
    assert down == set(range(1, 4 * VL + 1)) and up == set(range(-4 * VL, 0)), (sorted(down), sorted(up))


@pytest.mark.parametrize("Q", S.Q_LEVELS)
@pytest.mark.parametrize("VL", S.VECTOR_LEVELS)
def test_dark_flat_the_intra_cost_under_its_cap_loses_ties_and_wins(VL, Q):
    """see search_clips.dark_flat; every position class holds each of the three values"""
    c = S.census_of("dark_flat", VL, Q)
    clip, _ = S.dark_flat(VL)
    o = c["oracle"]
    assert (c["dump"]["recon"][0::2, :clip.shape[2] * clip.shape[3]] == S.DARK_REF).all()
    value = clip[1::2, 0, ::16, ::16].astype(np.int64)
    sad = 256 * (S.DARK_REF - value)
    hp = c["v10"][..., :9]
    assert (c["v10"][..., 9] == 256 * value).all() and ((hp == sad[..., None]) | (hp == 4096)).all() and (hp[..., 8] == 4096).all()
    assert (c["live"] == c["tie"]).all() and (c["tie"].sum(-1) >= (2 * VL + 1) ** 2).all()
    for k in S.KLASSES:
        at = np.broadcast_to(c["klass"] == S.KLASSES.index(k), value.shape)
        assert {int(v) for v in value[at]} == set(S.DARK_VALUES)
        last = max(S.legal_vectors(k, VL), key=lambda v: (v[1], v[0]))                    # the largest dy, then the largest dx
        m = at & (value == 11)
        assert (o["mb_inter"][m] == 1).all() and (o["mb_mvx"][m] == last[0]).all() and (o["mb_mvy"][m] == last[1]).all() and (c["idx"][m] == 4).all()
    assert (o["mb_inter"][value <= 10] == 0).all()


def test_the_census_tree_is_the_rtl_tree_over_every_tie_pattern():
    """search_clips.find_min_in_10_values (vectorised) against the scalar restatement of tests/rtl_stage_f.py, over every pattern of
    three values on ten inputs; among equal minima the winner is the first of 8, 9, 4, 5, 6, 7, 0, 1, 2, 3"""
    import rtl_stage_f
    v = np.array(list(itertools.product(range(3), repeat=10)))
    got = S.find_min_in_10_values(v)
    order = np.array(S.TREE_ORDER)
    first = order[(v[:, order] == v.min(1, keepdims=True)).argmax(1)]
    assert np.array_equal(got, first)
    for row, g in zip(v[::97], got[::97]):
        assert rtl_stage_f.find_min_in_10_values(list(row)) == g
