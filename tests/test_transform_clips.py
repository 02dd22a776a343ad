"""CPU: the oracle alone puts every clip of tests/transform_clips.py where tests/test_gpu_transform.py needs it - a coefficient on either
side of every boundary of the intra quantiser (levels 1, 2, 3 and the largest whose boundary the search reaches from 8-bit samples)
at every position, with both signs, in luma and in chroma, in I pictures and in intra macroblocks of P pictures; every residue of the DC coefficient in each of its
roles; either side of the boundaries of the non-intra quantiser at all 64 positions in luma and in chroma at every VECTOR_LEVEL; the
coefficients -2 .. 2 in coded tiles; negative levels whose product with an odd weight the inverse quantiser's shift has to floor; every
rounding class of the 2 x 2 chroma cells; the sums -1, 0, 255, 256 in front of the final clip, inverse transforms that leave their own clip range; mismatch control that toggles and does
not; every value of the two low byte limbs of the matrix cores' first pass.  All of it is computed by transform_clips.census from the
oracle's dump and its single-stage entries, and the first test here - the anchor - is that the census's levels and reconstruction are
the dump's on every macroblock of every clip, in default and in conformant mode (and that transform_clips.chain, the same arithmetic in
the form the kernel computes it, agrees with every stage of the census).  These are conditions on the generators as committed, asserted
on what the oracle produced and not on what a generator aimed at.  The last tests apply single-point faults to chain(): every one
changes a level or a reconstructed sample of the clips that are there for it.  numpy and the oracle only, but for the extremes clip:
test_gpu_extremes.basis_sign_frames, reused as it is, reads the basis from the built library's m2v_debug_table, and one test here loads
the library to assert that table equal to the oracle's.

Wall time (measured once): 64 s for the 191 cases - 35 s of it the census of the 42 cases in both modes (about 2700 tiles a picture through
the oracle's single-stage entries, one call each), 6 s the search for the largest levels."""
import numpy as np
import pytest

import transform_clips as T

CASES = T.cases()
TAB = T.tables()


def of_kind(kind, Q=None, VL=None):
    return [c for c in CASES if c[0] == kind and Q in (None, c[1]) and VL in (None, c[2])]


def missing(want, got):
    """the (position, C) of `want` whose key is not in `got` (transform_clips.reached)"""
    w = np.array(want)
    return [tuple(x) for x in w[~np.isin(T.keys(w[:, 0], w[:, 1]), got)].tolist()]


# ---------------------------------------------------------------------------------------------------------------------------------
# the anchor
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conformant", [False, True], ids=["default", "conformant"])
@pytest.mark.parametrize("case", CASES, ids=T.case_id)
def test_anchor_census_equals_the_oracles_levels_and_reconstruction_on_every_macroblock(case, conformant):
    c = T.census_of(*case, conformant)
    assert c["lev"].size > 0
    assert np.array_equal(c["lev"], c["coef"]), "levels: first difference at (picture, macroblock, tile, position) %s" % (np.argwhere(c["lev"] != c["coef"])[:1],)
    assert np.array_equal(c["recon"], c["rec"]), "reconstruction: first difference at %s" % (np.argwhere(c["recon"] != c["rec"])[:1],)
    ch = T.chain_of(c)                                  # the kernel's form of the same arithmetic, fault-free
    for k in ("C", "lev", "deq", "idct", "presum", "recon"):
        assert np.array_equal(ch[k].reshape(c[k].shape), c[k]), k
    # 4:4:4 -> 4:2:0: the dump's chroma is m2v_oracle_subsample of the clip's, and the numpy restatement's
    clip, H, W = T.cached_clip(*case)[0], c["H"], c["W"]
    for f in range(clip.shape[0]):
        for p in (1, 2):
            got = c["dump"]["yuv420"][f, W * H + (p - 1) * (W * H // 4):W * H + p * (W * H // 4)].reshape(H // 2, W // 2)
            assert np.array_equal(T.o_subsample(clip[f, p]), got) and np.array_equal(T.subsample_np(clip[f, p]), got)


def test_the_basis_the_extremes_clip_is_built_from_is_the_oracles():
    import m2v_load
    M = m2v_load.load()
    assert np.array_equal(np.array([M.lib().m2v_debug_table(0, i, j) for i in range(8) for j in range(8)]).reshape(8, 8), TAB["D"])


# ---------------------------------------------------------------------------------------------------------------------------------
# the intra quantiser
# ---------------------------------------------------------------------------------------------------------------------------------
def assert_boundaries(targets, Q, levels_of):
    """the targets come in fours (both signs below the boundary, both signs on it): m2v_oracle_quant takes them to -+(k - 1) and -+k"""
    t = np.array(targets).reshape(-1, 4, 2)
    C = np.zeros((t.shape[0] * 4, 64), np.int64)
    C[np.arange(len(C)), t[..., 0].reshape(-1)] = t[..., 1].reshape(-1)
    lev = levels_of(C)[np.arange(len(C)), t[..., 0].reshape(-1)].reshape(-1, 4)
    assert (lev[:, 0] == -lev[:, 1]).all() and (lev[:, 2] == -lev[:, 3]).all() and (lev[:, 2] == lev[:, 0] + 1).all() and (lev[:, 0] >= 0).all()
    return lev[:, 2]


@pytest.mark.parametrize("case", of_kind("intra"), ids=T.case_id)
def test_intra_ac_both_sides_of_the_boundaries_of_levels_1_2_3_at_every_position_in_luma_and_chroma(case):
    """756 of 756 (position, C) in luma tiles and in chroma tiles, at every Q_LEVEL and VECTOR_LEVEL; nothing left out"""
    Q = case[1]
    want = T.intra_ac_targets(Q)
    assert len(want) == 63 * 3 * 4
    k = assert_boundaries(want, Q, lambda C: T.o_quant(C, 0, Q))
    assert sorted(set(k.tolist())) == [1, 2, 3] and (np.bincount(k)[1:] == 63).all()
    c = T.census_of(*case)
    for chroma in (False, True):
        assert missing(want, T.reached(c, T.select(c, intra=True, chroma=chroma, p_picture=False), 1)) == []


@pytest.mark.parametrize("case", of_kind("intra_max"), ids=T.case_id)
def test_intra_ac_both_sides_of_the_boundary_of_the_largest_level(case):
    """MAX_LEVEL is what the search reaches (asserted), above 3 everywhere (Q_LEVEL 4, position 63: 5), and the clip holds its 252
    (position, C) in luma and in chroma"""
    Q = case[1]
    assert T.max_levels(Q) == T.MAX_LEVEL[Q] and min(T.MAX_LEVEL[Q][1:]) > 3
    want = T.intra_ac_targets(Q, levels=T.MAX_LEVEL[Q])
    k = assert_boundaries(want, Q, lambda C: T.o_quant(C, 0, Q))
    assert np.array_equal(k, T.MAX_LEVEL[Q][1:])
    c = T.census_of(*case)
    for chroma in (False, True):
        assert missing(want, T.reached(c, T.select(c, intra=True, chroma=chroma, p_picture=False), 1)) == []


@pytest.mark.parametrize("case", of_kind("intra", VL=1)[:2] + of_kind("intra_p")[:2], ids=T.case_id)
def test_negative_levels_times_every_odd_weight_that_the_inverse_quantisers_shift_has_to_floor(case):
    """Q_LEVEL 1 and 2: for every odd weight W a tile with a level q < 0 at a position of that weight and q W no multiple of 2^(3 - Q) -
    (q W) >> (3 - Q) rounds toward minus infinity there, a division toward zero gives one more - in luma and in chroma"""
    Q = case[1]
    assert Q in (1, 2)
    c = T.census_of(*case)
    odd = sorted(set(TAB["W"][1:][TAB["W"][1:] % 2 == 1].tolist()))
    assert odd == [19, 27, 29, 35, 37, 69, 83]
    for chroma in (False, True):
        lev = c["lev"][T.select(c, intra=True, chroma=chroma, p_picture=case[0] == "intra_p")]
        prod = lev * TAB["W"]
        hit = (lev < 0) & (prod % (1 << (3 - Q)) != 0)
        hit[:, 0] = False
        assert sorted(set(np.broadcast_to(TAB["W"], hit.shape)[hit].tolist()) & set(odd)) == odd


DC_ROLES = (("Y00", (0,)), ("chained luma", (1, 2, 3)), ("U", (4,)), ("V", (5,)))


def assert_dc_residues(c, p_picture):
    m = T.select(c, intra=True, p_picture=p_picture)
    for name, tiles in DC_ROLES:
        C = np.concatenate([c["C"][:, :, t, 0][m[:, :, t]] for t in tiles])
        got = set(zip(np.sign(C).tolist(), (np.abs(C) % 16).tolist()))
        assert got >= {(s, r) for s in (-1, 1) for r in range(16)}, name
        assert C.min() == -8192 and C.max() == 8128, name          # flat 0 and flat 255: 64 (0 - 128), 64 (255 - 128)


@pytest.mark.parametrize("case", of_kind("intra"), ids=T.case_id)
def test_intra_dc_every_residue_mod_16_of_both_signs_in_each_role_and_flat_0_and_255(case):
    """|C| mod 16 = 0 .. 15 for C > 0 and C < 0 (the rounding bit is bit 3), as Y00, as a chained luma tile, as U and as V; C = -8192
    and 8128 are the smallest and largest there are"""
    assert_dc_residues(T.census_of(*case), False)


# ---------------------------------------------------------------------------------------------------------------------------------
# the non-intra quantiser
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of_kind("inter"), ids=T.case_id)
def test_inter_both_sides_of_the_boundaries_of_levels_1_2_3_at_all_64_positions_in_luma_and_chroma(case):
    """768 of 768 (position, C), |C| = (k << (4 + Q)) - 3 and - 2, in luma tiles (matrix cores) and in chroma tiles (VALU path) of
    non-intra macroblocks, at every Q_LEVEL and VECTOR_LEVEL; every macroblock of the picture is non-intra with the zero vector"""
    Q = case[1]
    want = T.inter_targets(Q)
    assert len(want) == 64 * 3 * 4
    k = assert_boundaries(want, Q, lambda C: T.o_quant(C, 1, Q))
    assert (np.bincount(k)[1:] == 64).all() and len(np.bincount(k)) == 4
    c = T.census_of(*case)
    assert c["inter"][1].all() and not c["dump"]["mb_mvx"][1].any() and not c["dump"]["mb_mvy"][1].any()
    for chroma in (False, True):
        assert missing(want, T.reached(c, T.select(c, intra=False, chroma=chroma, p_picture=True))) == []


@pytest.mark.parametrize("conformant", [False, True], ids=["default", "conformant"])
@pytest.mark.parametrize("case", of_kind("inter"), ids=T.case_id)
def test_inter_coefficients_minus_2_to_2_in_coded_tiles_and_tiles_without_levels_beside_coded_ones(case, conformant):
    """C = -2, -1 (where the sign of C + 2 is not the sign of C), 0, 1, 2 at some position of a coded tile, luma and chroma; and tiles
    whose every level is 0 in macroblocks with coded tiles: pattern bit 0, and in conformant mode not reconstructed at all"""
    c = T.census_of(*case, conformant)
    for chroma in (False, True):
        m = T.select(c, intra=False, chroma=chroma, p_picture=True)
        C, lev = c["C"][m], c["lev"][m]
        coded = lev.any(1)
        assert set(range(-2, 3)) <= set(np.unique(C[coded]).tolist())
    empty = ~c["lev"].any(3) & c["inter"][:, :, None]
    beside = empty & (~empty).any(2)[:, :, None]
    assert beside[1][:, :4].any() and beside[1].sum() >= 100
    assert not c["idct"][beside].any() and np.array_equal(c["rec"][beside], c["pred"][beside])


# ---------------------------------------------------------------------------------------------------------------------------------
# intra macroblocks in P pictures
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of_kind("intra_p"), ids=T.case_id)
def test_intra_macroblocks_of_a_p_picture_level_1_boundaries_at_every_position_and_every_dc_residue(case):
    """252 of 252 (position, C) of level 1 in luma (matrix cores) and in chroma (VALU path, the intra constants fetched inside the
    branch) of intra macroblocks of a P picture - every macroblock of it is intra - and the DC residues in each role"""
    Q = case[1]
    want = T.intra_ac_targets(Q, ks=(1,))
    assert (assert_boundaries(want, Q, lambda C: T.o_quant(C, 0, Q)) == 1).all()
    c = T.census_of(*case)
    assert list(c["p_picture"]) == [False, True, True] and not c["inter"][1].any()
    for chroma in (False, True):
        assert missing(want, T.reached(c, T.select(c, intra=True, chroma=chroma, p_picture=True), 1)) == []
    assert_dc_residues(c, True)


# ---------------------------------------------------------------------------------------------------------------------------------
# subsampling
# ---------------------------------------------------------------------------------------------------------------------------------
def test_subsampling_every_rounding_class_of_the_cells_and_the_dc_level_names_the_sample():
    """chroma tiles of one cell (a, b / c, d) each: all eight parities of (a + b, c + d, h0 + h1); cells where the two stages give one
    more than (a + b + c + d + 2) >> 2; cells of 0 and of 255; and the tile's DC level is 4 (s - 128) with s the two-stage value.
    The two stages never give LESS than the single rounding (each stage rounds up, so s >= the exact mean, and the single rounding is at
    most its ceiling): asserted here over every cell of 0 .. 7, so that direction has no clip."""
    (case,) = of_kind("subsample")
    c = T.census_of(*case)
    clip = T.cached_clip(*case)[0]
    mbw = c["W"] // 16
    par, diff, cells = set(), set(), set()
    for mb in range(c["inter"].shape[1]):
        by, bx = divmod(mb, mbw)
        for p in (1, 2):
            blk = clip[0, p, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16].astype(np.int64)
            a, b, cc, d = (int(v) for v in blk[:2, :2].reshape(-1))
            assert np.array_equal(blk, np.kron(np.ones((8, 8), np.int64), blk[:2, :2]))
            h0, h1 = (a + b + 1) >> 1, (cc + d + 1) >> 1
            s = (h1 + h0 + 1) >> 1
            assert (c["cur"][0, mb, 3 + p] == s).all() and c["lev"][0, mb, 3 + p, 0] == 4 * (s - 128) and not c["lev"][0, mb, 3 + p, 1:].any()
            par.add(((a + b) % 2, (cc + d) % 2, (h0 + h1) % 2))
            diff.add(s - ((a + b + cc + d + 2) >> 2))
            cells.add((a, b, cc, d))
    assert len(par) == 8 and diff == {0, 1} and (0,) * 4 in cells and (255,) * 4 in cells
    g = np.stack(np.meshgrid(*[np.arange(8)] * 4, indexing="ij"), -1).reshape(-1, 2, 2)
    two = np.array([T.subsample_np(x)[0, 0] for x in g])
    assert (two >= (g.sum((1, 2)) + 2) >> 2).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the final clip
# ---------------------------------------------------------------------------------------------------------------------------------
CLIP_GROUPS = [(intra, p, chroma) for intra, p in ((True, False), (True, True), (False, True)) for chroma in (False, True)]


@pytest.mark.parametrize("conformant", [False, True], ids=["default", "conformant"])
def test_the_sum_in_front_of_the_final_clip_is_minus_1_0_255_and_256(conformant):
    """prediction + idct takes each of -1, 0, 255, 256 in intra macroblocks of I pictures, in intra macroblocks of P pictures and in
    non-intra macroblocks, in luma and in chroma - over the clipper clips, printed per clip"""
    got = {g: set() for g in CLIP_GROUPS}
    for case in of_kind("clipper"):
        c = T.census_of(*case, conformant)
        for g in CLIP_GROUPS:
            v = set(np.unique(c["presum"][T.select(c, intra=g[0], p_picture=g[1], chroma=g[2])]).tolist()) & {-1, 0, 255, 256}
            print(T.case_id(case), g, sorted(v))
            got[g] |= v
    assert all(v == {-1, 0, 255, 256} for v in got.values()), got


@pytest.mark.parametrize("conformant", [False, True], ids=["default", "conformant"])
def test_the_inverse_transform_leaves_its_own_clip_range_in_both_directions(conformant):
    """what the column pass hands to the clip of RTL:778-783 (-255 .. 255; conformant: -256 .. 255) lies below and above that range - the
    sum with the prediction is then below -255 + prediction and above 255 + prediction - in non-intra tiles of luma (clipper: a
    flipped 4 x 4 patch) and of chroma (extremes), and in intra tiles (intra_over: the two recorded blocks, -259 and +257 at Q_LEVEL 4)
    of luma and of chroma, in the I picture and in intra macroblocks of the P picture.  k_mb leaves that clip out, because the final clip
    gives the same sample (prediction + r <= 0 for every r <= -255, >= 255 for every r >= 255): asserted on every such sample"""
    lo = -256 if conformant else -255
    groups = [(False, None, chroma) for chroma in (False, True)] + [(True, p, chroma) for p in (False, True) for chroma in (False, True)]
    below, above = {g: 0 for g in groups}, {g: 0 for g in groups}
    for case in of_kind("clipper") + of_kind("extremes") + of_kind("intra_over"):
        c = T.census_of(*case, conformant)
        raw = T.chain_of(c)["idct_raw"].reshape(c["idct"].shape)
        assert np.array_equal(np.clip(raw, lo, 255), c["idct"])
        for g in groups:
            m = T.select(c, intra=g[0], p_picture=g[1], chroma=g[2])
            below[g] += int((raw[m] < lo).sum())
            above[g] += int((raw[m] > 255).sum())
            assert (c["presum"][m][raw[m] < lo] == c["pred"][m][raw[m] < lo] + lo).all() and (c["rec"][m][raw[m] < lo] == 0).all()
            assert (c["presum"][m][raw[m] > 255] == c["pred"][m][raw[m] > 255] + 255).all() and (c["rec"][m][raw[m] > 255] == 255).all()
    print("samples below / above the range, {(intra, P picture, chroma): count}:", below, above)
    assert all(below.values()) and all(above.values())


def test_the_recorded_blocks_overshoot_by_what_their_comment_says():
    """OVER_BLOCKS through the oracle's fdct / quant / dequant and the unclipped column pass: -259 and +257 at sample 0, both modes"""
    x = np.array(T.OVER_BLOCKS) - 128
    for conformant in (False, True):
        deq = T.o_dequant(T.o_quant(T.o_fdct(x), 0, T.OVER_Q), 0, T.OVER_Q, conformant)
        raw = T.idct_np(deq, conformant, clip=False)
        assert np.array_equal(np.clip(raw, -256 if conformant else -255, 255), T.o_idct(deq, conformant))
        assert raw[0, 0] == raw[0].min() == -259 and raw[1, 0] == raw[1].max() == 257


# ---------------------------------------------------------------------------------------------------------------------------------
# the conformant inverse quantiser
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", of_kind("intra", VL=1) + of_kind("inter", VL=1) + of_kind("intra_p"), ids=T.case_id)
def test_mismatch_control_toggles_and_does_not_and_makes_coefficient_63_non_zero(case):
    """conformant mode: coded tiles whose dequantised sum is even (coefficient 63 toggles) and, where there are any, odd (it does not),
    and tiles where the toggle makes coefficient 63 +1 from a level of 0.  An odd sum exists only in intra tiles at Q_LEVEL 1 .. 3: with
    the quantiser_scale 2 << Q that the slice header carries, a non-intra coefficient is (2 q + sign) << Q and an intra one at Q_LEVEL 4
    is 2 q W, every one even (asserted) - there every coded tile toggles"""
    c = T.census_of(*case, True)
    ch = T.chain_of(c)
    assert np.array_equal(ch["deq"].reshape(c["deq"].shape), c["deq"])
    tog = ch["toggled"].reshape(c["lev"].shape[:3])
    m = T.select(c, intra=case[0] != "inter", p_picture=case[0] != "intra") & c["lev"].any(3)
    if case[0] == "inter" or case[1] == 4:
        assert tog[m].all() and (c["deq"][m][:, :63] % 2 == 0).all()
    else:
        assert tog[m].any() and (~tog[m]).any()
    from_zero = m & tog & (c["lev"][..., 63] == 0)
    assert from_zero.any() and (c["deq"][..., 63][from_zero] == 1).all()


# ---------------------------------------------------------------------------------------------------------------------------------
# the byte limbs of the matrix cores' first pass
# ---------------------------------------------------------------------------------------------------------------------------------
LIMB_HIGH = (127, 129)          # the high byte of T + 0x808080 over the luma tiles of the extremes clips: smallest, largest


def test_the_two_low_limbs_take_all_256_values_and_the_high_limb_what_the_extremes_clip_gives_it():
    """T = Z . B16^T restated from m2v_oracle_tab_dct over the luma tiles of every clip: each of the two low bytes of T + 0x808080 takes
    all 256 values, the high byte lies in the range the full-swing basis patterns give it and reaches both ends"""
    seen = [np.zeros(256, bool) for _ in range(3)]
    high = {}
    for case in [c for c in CASES if c[2] == 3 or c[0] not in ("intra", "inter")]:
        c = T.census_of(*case)
        b, s = T.limbs(T.first_pass(c["resid"][:, :, :4].reshape(-1, 64)))
        assert np.array_equal(s[0] + (s[1] << 8) + (s[2] << 16), T.first_pass(c["resid"][:, :, :4].reshape(-1, 64)))
        for k in range(3):
            seen[k][np.unique(b[k])] = True
        high.setdefault(case[0], set()).update(np.unique(b[2]).tolist())
    print("high byte per kind of clip:", {k: (min(v), max(v)) for k, v in high.items()})
    assert seen[0].all() and seen[1].all()
    assert (min(high["extremes"]), max(high["extremes"])) == LIMB_HIGH
    assert (int(np.flatnonzero(seen[2]).min()), int(np.flatnonzero(seen[2]).max())) == LIMB_HIGH


# ---------------------------------------------------------------------------------------------------------------------------------
# single-point faults of the kernel's form of the arithmetic
# ---------------------------------------------------------------------------------------------------------------------------------
def faulty_levels(c, fault, position=None):
    """-> bool, the census's shape: where the levels of quant_np with the fault are not the oracle's"""
    lev = T.quant_np(c["C"].reshape(-1, 64), np.repeat(c["inter"][:, :, None], 6, 2).reshape(-1), c["Q"], fault, position)
    return lev.reshape(c["lev"].shape) != c["lev"]


@pytest.mark.parametrize("case", of_kind("intra", VL=1) + of_kind("intra_p"), ids=T.case_id)
def test_fault_one_reciprocal_of_the_intra_quantiser_one_too_small(case):
    """ceil(2^21 / W) - 1 at ONE position, every position in turn: a level changes in a luma tile and in a chroma tile (and nowhere
    but at that position)"""
    c = T.census_of(*case)
    for p in range(1, 64):
        d = faulty_levels(c, "recip", p)
        assert not np.delete(d, p, 3).any()
        for chroma in (False, True):
            assert d[T.select(c, intra=True, chroma=chroma, p_picture=case[0] == "intra_p")][:, p].any(), (p, chroma)


@pytest.mark.parametrize("fault,kinds", [("qoff_shift", ("intra", "intra_p", "intra_max")), ("dc_rounding", ("intra", "intra_p")), ("inter_bias", ("inter",))])
def test_fault_in_a_quantiser_changes_a_level_of_every_clip_that_is_there_for_it(fault, kinds):
    """qoff with >> 2, the DC coefficient truncated, the bias of a negative non-intra value one too large: luma and chroma"""
    for case in [c for c in CASES if c[0] in kinds]:
        c = T.census_of(*case)
        d = faulty_levels(c, fault)
        for chroma in (False, True):
            assert d[T.select(c, chroma=chroma)].any(), (case, chroma)


@pytest.mark.parametrize("fault,kinds", [("dequant_toward_zero", ("intra", "intra_p")), ("clip_254", ("intra", "intra_p", "clipper")), ("middle_limb", ("intra", "inter", "intra_p", "clipper"))])
def test_fault_behind_the_quantiser_changes_a_reconstructed_sample_or_a_level(fault, kinds):
    """the inverse quantiser's shift toward zero (Q_LEVEL 1 and 2: from 3 on it shifts left), the final clip at 254, the middle limb of
    the first pass recombined without its sign flip"""
    for case in [c for c in CASES if c[0] in kinds and (fault != "dequant_toward_zero" or c[1] <= 2)]:
        c = T.census_of(*case)
        ch = T.chain_of(c, fault)
        changed = (ch["recon"].reshape(c["recon"].shape) != c["recon"]) | (ch["lev"].reshape(c["lev"].shape) != c["lev"])
        groups = (False,) if fault == "middle_limb" else (False, True)          # the limbs are the luma tiles' (and an I picture's chroma)
        for chroma in groups:
            assert changed[T.select(c, chroma=chroma)].any(), (case, chroma)


def test_fault_one_stage_subsampling_changes_a_sample():
    (case,) = of_kind("subsample")
    c = T.census_of(*case)
    clip, H, W = T.cached_clip(*case)[0], c["H"], c["W"]
    got = c["dump"]["yuv420"][0, W * H:W * H * 5 // 4].reshape(H // 2, W // 2)
    assert np.array_equal(T.subsample_np(clip[0, 1]), got) and not np.array_equal(T.subsample_np(clip[0, 1], "one_stage_subsampling"), got)
