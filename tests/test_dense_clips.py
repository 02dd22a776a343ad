"""CPU: the oracle alone puts every clip of tests/dense_clips.py where tests/test_gpu_dense_wide.py needs it - all four slot classes
in every slice, the staging of k_assemble filling inside the slice, macroblock sizes on both sides of every class boundary, slices of
many passes.  These are conditions on the generators as committed (figures measured when they were written are in the comments); a
retuned generator that misses one fails here, on the CPU, instead of leaving a GPU test that no longer reaches its code path.
numpy and the oracle only."""
import numpy as np
import pytest

import dense_clips as D
from oracle import m2v_oracle_ctypes as orc


def dump(clip, pf, VL=3, Q=2):
    n, _, H, W = clip.shape
    _, d = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, dump=True)
    return d


@pytest.mark.parametrize("pf", [0, 3])
@pytest.mark.parametrize("seed", [11, 12])
@pytest.mark.parametrize("mbw,ys16", [(120, 4), (127, 4), (128, 4), (128, 8)])
def test_mix_every_slice_holds_all_four_classes_and_overfills_the_staging(mbw, ys16, seed, pf):
    """measured minima over every slice: 9 / 5 / 19 / 19 macroblocks per class, 1168 staged words; slices of 12 - 19 KB (3 - 5 passes)"""
    d = dump(D.mix(16 * mbw, 16 * ys16, 4, seed), pf)
    s = D.describe(d["mb_bits"], mbw)
    print("mix %d x %d seed %d pf %d: class minima %s, staged words %d..%d, slice bytes %d..%d" % (
        mbw, ys16, seed, pf, s["classes"].min(0), s["staged_words"].min(), s["staged_words"].max(), s["slice_bytes"].min(), s["slice_bytes"].max()))
    assert (s["classes"] >= 4).all(), s["classes"].min(0)
    assert (s["staged_words"] > D.STAGE_WORDS).all(), s["staged_words"].min()
    assert (s["slice_bytes"] > 2 * D.IMAGE_BYTES).all()
    if pf:
        assert d["mb_inter"][1:].any() and not d["mb_inter"][1:].all()


@pytest.mark.parametrize("pf", [0, 3])
@pytest.mark.parametrize("mbw", [33, 63, 64, 65])
def test_mix_narrower_widths_hold_every_class(mbw, pf):
    """under 120 macroblocks the staging need not fill and a slice may miss a class: over the whole clip every class is there"""
    s = D.describe(dump(D.mix(16 * mbw, 64, 4, 11), pf)["mb_bits"], mbw)
    assert (s["classes"].sum(0) >= 4).all(), s["classes"].sum(0)


def wide_short_dump(mbw, content, Q, pf, ys16=4):
    """what tests/test_gpu_dense_wide.py::test_wide_and_short_dense_slices runs for these parameters"""
    assert (mbw, ys16, content, 3, Q, pf) in D.wide_short_cases()
    return dump(D.wide_short_clip(mbw, ys16, content, Q), pf, Q=Q)


@pytest.mark.parametrize("pf", [0, 3])
def test_noise_at_q4_33_wide_is_within_a_macroblock_of_the_staging(pf):
    """33 nearly full compact slots (842 - 1009 bits): measured 980 - 1056 staged words per slice by mb_bits, on both sides of the 1024 -
    the condition as it was set for this clip.  By the exact count (printed) it is 984 - 1020 for both pframes: on the GPU this clip
    stays just UNDER the staging in every slice; "brim" below is the one that crosses it."""
    d = wide_short_dump(33, "noise", 4, pf)
    s = D.describe(d["mb_bits"], 33)
    print("noise Q 4 at 33: staged words by mb_bits %s, exact %s" % (sorted(s["staged_words"].tolist()), sorted(D.staged_words_exact(d, 33, pf)[0].tolist())))
    assert d["mb_bits"].min() > 560 and d["mb_bits"].max() < 1100
    assert (s["staged_words"] > D.STAGE_WORDS).any() and (s["staged_words"] <= D.STAGE_WORDS).any(), sorted(s["staged_words"])


def test_brim_at_33_fills_the_staging_at_the_last_macroblock_by_the_kernels_own_count():
    """the exact count (slot_bits: mb_bits less the neighbour-dependent codes), compact slots only.  Measured, I-only: 12 slices of 20
    over the 1024 words, 8 under, no overflow slot anywhere; I+P: 5 over and 3 under among the slices without an overflow slot"""
    d = wide_short_dump(33, "brim", 2, 0)
    staged, big = D.staged_words_exact(d, 33, 0)
    print("brim, I-only: staged words %s" % sorted(staged.tolist()))
    assert (big == 0).all()
    assert (staged > D.STAGE_WORDS).sum() >= 4 and (staged <= D.STAGE_WORDS).sum() >= 4
    assert staged.max() <= D.STAGE_WORDS + 32            # ... by the last macroblock alone
    d = wide_short_dump(33, "brim", 2, 3)
    staged, big = D.staged_words_exact(d, 33, 3)
    assert ((big == 0) & (staged > D.STAGE_WORDS)).sum() >= 2 and ((big == 0) & (staged <= D.STAGE_WORDS)).sum() >= 2


@pytest.mark.parametrize("mbw,pf", [(64, 0), (65, 3), (128, 0), (128, 3)])
def test_noise_at_q4_is_compact_slots_only_and_overfills_the_staging_mid_slice(mbw, pf):
    """every macroblock 26 - 31 words by the exact count: the staging is full after 33 - 39 macroblocks, the rest of the slice is read
    from memory, and no overflow slot is involved (measured: 1904 - 1956 staged words at 64, 3824 - 3896 at 128)"""
    d = wide_short_dump(mbw, "noise", 4, pf)
    staged, big = D.staged_words_exact(d, mbw, pf)
    assert (big == 0).all()
    assert (staged > D.STAGE_WORDS + 256).all(), staged.min()


@pytest.mark.parametrize("mbw,pf", [(120, 0), (120, 3), (127, 0), (127, 3), (128, 0), (128, 3)])
def test_mix_by_the_kernels_own_count(mbw, pf):
    """the mix clip as the GPU test runs it: by the exact count every slice over-fills the staging (measured 1336 - 2076 words) and holds
    overflow slots as well (19 - 49)"""
    d = wide_short_dump(mbw, "mix", 2, pf)
    staged, big = D.staged_words_exact(d, mbw, pf)
    assert (staged > D.STAGE_WORDS).all() and (big >= 4).all(), (staged.min(), big.min())
    words = (D.slot_bits(d, mbw, pf).reshape(-1, mbw) + 31) // 32
    for lo, hi in ((0, 8), (9, 16), (17, 32)):
        assert (((words >= lo) & (words <= hi)).sum(1) >= 4).all(), (lo, hi)


def test_slot_bits_of_flat_pictures():
    """known answers for slot_bits: a flat intra macroblock keeps 3 luma DC codes of size 0 (3 bits each) and 6 end-of-block codes
    (2 bits each) in its slot; an inter macroblock without coefficients keeps nothing"""
    d = dump(D.flat(64, 64, 2), 1)
    sb = D.slot_bits(d, 4, 1)
    assert (sb[0] == 21).all() and (d["mb_bits"][0] == 30).all()
    assert d["mb_inter"][1].all() and (sb[1] == 0).all()


@pytest.mark.parametrize("Q,pf", [(2, 3), (1, 3), (2, 0)])
def test_ramp_samples_every_class_boundary(Q, pf):
    """the 128 x 8 ramp cases of the GPU test (5 frames, seed 11).  Measured: 57 / 65 / 71 distinct sizes in the windows at Q 2 with
    pframes 3 (of 66 / 66 / 71 possible), 54 / 63 / 70 at Q 1, 64 / 63 / 71 at Q 2 I-only; 2389 of 3072 P macroblocks inter at Q 2.  The narrower and 4-row ramp cases
    sample fewer sizes (11 - 51 per window) and the Q 4 ones stop short of the 1024-bit boundary; nothing is asserted for them."""
    d = wide_short_dump(128, "ramp", Q, pf, ys16=8)
    s = D.describe(d["mb_bits"], 128)
    inter = d["mb_inter"][[1, 2, 3]] if pf else d["mb_inter"][:0]
    print("ramp 128 x 8 Q %d pframes %d: distinct sizes in the windows %s, %d of %d P macroblocks inter" % (
        Q, pf, s["window_values"], int(inter.sum()), inter.size))
    assert min(s["window_values"]) >= 45, s["window_values"]
    if pf:
        assert 4 * int(inter.sum()) >= inter.size


@pytest.mark.parametrize("pf", [0, 3])
def test_binary_noise_at_q1_slices_take_more_than_eight_passes(pf):
    """measured: every macroblock 4039 - 4485 bits, every slice 67.8 - 68.2 KB = 17 passes over the 4 KB image"""
    d = dump(D.binary_noise(2048, 64, 4, 5), pf, Q=1)
    s = D.describe(d["mb_bits"], 128)
    assert (s["slice_bytes"] > 8 * D.IMAGE_BYTES).all(), s["slice_bytes"].min()
    assert d["mb_bits"].min() > 1100
    assert (s["classes"][:, 3] == 128).all()


def test_checker_is_dense_at_every_q():
    """the checkerboards are uniform: every macroblock of a picture has the same size but for its header codes (measured 1330 bits at
    Q 1, 1082 at Q 2 - overflow slots just past the 1024-bit boundary -, figures printed)"""
    for Q in (1, 2, 4):
        b = dump(D.checker(2048, 64, 2), 0, Q=Q)["mb_bits"]
        print("checker Q %d: %d..%d bits per macroblock" % (Q, b.min(), b.max()))
        assert b.max() - b.min() <= 8
        if Q == 1:
            assert b.min() > 1100


def test_largest_macroblock_the_generators_produce():
    """A printed fact, not a threshold: the largest macroblock against the 9728-bit slot, for the generators' clips and for a short
    seeded search: 8x8 tiles of full-swing sign patterns (every sample 0 or 255, the density of 255s drawn per tile), as an intra
    picture and as a P picture over its complement (residual +-255)."""
    gen = {"binary_noise": D.binary_noise(2048, 64, 4, 5), "noise": D.noise(2048, 64, 2, 5), "checker": D.checker(2048, 64, 2), "mix": D.mix(2048, 64, 2, 11)}
    gen = {name: max(int(dump(clip, pf, Q=1)["mb_bits"].max()) for pf in (0, 3)) for name, clip in gen.items()}
    rng = np.random.default_rng(77)
    search = (0, "")
    for t in range(200):
        p = rng.uniform(0.2, 0.8, (1, 3, 8, 8))
        f0 = (rng.random((1, 3, 64, 64)) < np.kron(p, np.ones((8, 8)))).astype(np.uint8) * 255
        clip = np.concatenate([f0, 255 - f0]).astype(np.uint8)
        for pf in (0, 1):
            search = max(search, (int(dump(clip, pf, VL=1, Q=1)["mb_bits"].max()), "try %d, pframes %d" % (t, pf)))
    print("largest macroblock, bits: generators %s; sign pattern search %d (%s); the slot holds %d" % (gen, search[0], search[1], D.SLOT_BITS))
    assert max(max(gen.values()), search[0]) <= D.SLOT_BITS          # what k_mb's overflow slot relies on (csrc/m2v_types.hpp kSlotWords)


def test_the_case_list_covers_what_it_claims():
    """tests/test_gpu_dense_wide.py thins width x content x Q x pframes: every width still meets every content, binary noise at Q 1
    meets 128 macroblocks I-only and I+P, the mix clip meets every VECTOR_LEVEL"""
    from dense_clips import CONTENTS, WIDTHS
    cases = D.wide_short_cases()
    for mbw in WIDTHS:
        for content in CONTENTS:
            assert any(c[0] == mbw and c[2] == content for c in cases), (mbw, content)
    assert {(c[4], c[5]) for c in cases if c[:4] == (128, 4, "binary", 3)} >= {(1, 0), (1, 3)}
    assert {c[4] for c in cases} == {1, 2, 4} and {c[5] for c in cases} == {0, 3}
    assert {c[3] for c in cases if c[2] == "mix"} == {1, 2, 3}
