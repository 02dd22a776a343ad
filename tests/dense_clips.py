"""Seeded dense clips for wide frames, and what the oracle's mb_bits dump says about them.

tests/corner_clips.py builds clips for corners of the arithmetic; these are for the stream assembly (csrc/m2v_kernels.hpp k_mb's slot
classes, k_assemble's staging and passes) and for the buffers behind it.  k_mb stores a macroblock's bits in a slot of 8, 16 or 32
words, or in the 304-word overflow slot; k_assemble stages the compact slots of a slice in 1024 words of LDS, reads what found no
room there (and every overflow slot) from memory, and builds the slice in passes of 4 KB.  synth.clip's content leaves nearly every
macroblock in the two smallest classes and every slice in one pass; white noise on the narrow frames of the other tests puts every
macroblock of a slice in ONE class.  The clips here mix the classes inside a slice of 33 .. 128 macroblocks:

  noise(W, H, n, seed)            uniform samples 0..255, all three planes
  binary_noise(W, H, n, seed)     every sample 0 or 255: the densest content made of pixels that was found (see below)
  checker(W, H, n)                synth.degenerate("checker"): full-swing checkerboards of three phases
  mix(W, H, n, seed, amps)        every 16x16 macroblock of every frame draws an amplitude a from `amps`; its samples are
                                  clip(128 + (u - 128) * a // 255), u uniform in 0..255.  With (0, 28, 64, 255) at Q_LEVEL 2 the four
                                  amplitudes land in the four slot classes.
  ramp(W, H, n, seed, amax)       the same with a uniform in 0..amax: macroblock sizes sweep across the class boundaries
  flat(W, H, n, value)            constant planes (the sparse end: a few bytes per slice)
  mix(..., amps=BRIM_AMPS)        "brim": every macroblock a compact slot of 26 - 32 words at Q_LEVEL 2 - 33 of them fill the staging to
                                  the brim: just over in some slices, just under in others

describe(mb_bits, mbw) derives from the oracle's dump alone what the GPU tests rely on; tests/test_dense_clips.py (CPU) asserts it for
the clips as committed, so that a GPU test cannot go vacuous when a generator is retuned.  Classes are taken with margins (<= 200,
300 - 480, 560 - 990, >= 1100 bits): the oracle's mb_bits include the neighbour-dependent header codes (motion vector deltas, DC
differentials, address increment), which the kernel keeps outside the slot; the margins keep a macroblock's class independent of them.
slot_bits(dump, mbw, pframes) takes those codes off again (13 - 45 bits per macroblock of noise) and staged_words_exact() adds up what
the kernel's scan adds up: where a slice is within a few words of the 1024, only that count says on which side it is.  Uniform noise
at Q_LEVEL 4 on 33 macroblocks is 980 - 1056 words per slice by mb_bits, on both sides, but 984 - 1020 by the exact count: it stays
under the staging in every slice, and "brim" (1008 - 1044) is the clip that crosses it at that width.
tests/test_gpu_dense_wide.py::test_slot_bits_is_what_k_mb_stored pins slot_bits against the record k_mb itself leaves (m2v_debug_read 5).

wide_short_cases() is the thinned width x content x Q x pframes product the GPU test runs and wide_short_clip() the clip of a case:
kept here so that the CPU conditions are asserted on the very clips the GPU encodes.

Largest macroblock: the binary-noise clips at Q_LEVEL 1 give 4039 - 4485 bits per macroblock (uniform noise 2900 - 3600).
tests/test_dense_clips.py::test_largest_macroblock_the_generators_produce prints the largest macroblock of the generators' clips and
that of a short seeded search over per-tile sign patterns (200 tries, intra and over the complement) next to the 9728-bit slot
(304 words): 4485 bits for binary noise (I + P), and the search ends at the same 4485, no higher - under half of the slot.  Nothing
made of pixels came near the slot size."""
import ctypes

import numpy as np

import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()

MIX_AMPS = (0, 28, 64, 255)
BRIM_AMPS = (62, 64)                 # at Q_LEVEL 2: slots of 26 - 32 words, so that 33 of them add up to just under or just over the staging
CLASS_BITS = ((0, 200), (300, 480), (560, 990), (1100, 1 << 30))      # margined: micro (<= 8 words), tiny (<= 16), small (<= 32), overflow
WINDOWS = ((225, 290), (480, 545), (990, 1060))                       # around the 256 / 512 / 1024-bit class boundaries
STAGE_WORDS = 1024                                                    # kAsmStageWords
IMAGE_BYTES = 4096                                                    # kAsmImageWords * 4
SLOT_BITS = 304 * 32                                                  # kSlotWords

WIDTHS = (33, 63, 64, 65, 120, 127, 128)         # macroblocks per slice: just past the staging with full compact slots; around the
CONTENTS = ("binary", "mix", "ramp", "checker")  # wavefront boundary of the scans; config c3's width; the last thread idle; every thread used
# ramp amplitudes: at Q_LEVEL 1 and 2 the sizes sweep all three class boundaries (asserted for the 128 x 8 cases, tests/test_dense_clips.py);
# at Q_LEVEL 4 the largest amplitude there is ends at about 1000 bits: the 256- and 512-bit boundaries only, no overflow slot
RAMP_AMAX = {1: 40, 2: 80, 3: 120, 4: 255}
WIDE_SHORT_FRAMES = 5                            # with pframes 3 a whole GOP and the I frame of the next


def noise(W, H, n, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, 3, H, W), dtype=np.uint8)


def binary_noise(W, H, n, seed):
    return (np.random.default_rng(seed).integers(0, 2, (n, 3, H, W), dtype=np.uint8) * 255).astype(np.uint8)


def checker(W, H, n):
    return M.synth.degenerate("checker", W, H, n)


def flat(W, H, n, value=128):
    return np.full((n, 3, H, W), value, np.uint8)


def _scaled_noise(rng, amp, W, H, n):
    """amp: [n, H/16, W/16] amplitudes -> clip(128 + (u - 128) * a // 255) per sample, the same amplitude on all three planes"""
    u = rng.integers(0, 256, (n, 3, H, W)).astype(np.int64)
    a = np.kron(amp, np.ones((16, 16), np.int64))[:, None]
    return np.clip(128 + (u - 128) * a // 255, 0, 255).astype(np.uint8)


def mix(W, H, n, seed, amps=MIX_AMPS):
    rng = np.random.default_rng(seed)
    amp = rng.choice(np.asarray(amps, np.int64), (n, H // 16, W // 16))
    return _scaled_noise(rng, amp, W, H, n)


def ramp(W, H, n, seed, amax=80):
    rng = np.random.default_rng(seed)
    amp = rng.integers(0, amax + 1, (n, H // 16, W // 16))
    return _scaled_noise(rng, amp, W, H, n)


def make_clip(content, W, H, n, seed, Q=2):
    if content == "binary":
        return binary_noise(W, H, n, seed)
    if content == "noise":
        return noise(W, H, n, seed)
    if content == "mix":
        return mix(W, H, n, seed)
    if content == "brim":
        return mix(W, H, n, seed, amps=BRIM_AMPS)
    if content == "ramp":
        return ramp(W, H, n, seed, RAMP_AMAX[Q])
    if content == "checker":
        return checker(W, H, n)
    if content == "synth":
        return M.synth.clip(W, H, n, clip_index=seed)
    if content == "flat":
        return flat(W, H, n)
    raise ValueError(content)


def wide_short_cases():
    """(mbw, ys16, content, VL, Q, pframes): every width meets every content with both pframes; Q cycles over the product, except that
    from 120 macroblocks on the mix clip keeps Q 2 (where it holds all four classes) and the ramp clip Q 1 or 2 (where it reaches all
    three boundaries; 8 rows at 128); binary noise at Q 1 meets 128 both ways.  Then the cases whose slices hold compact slots ONLY, so
    that nothing but the staged / unstaged boundary is at work: uniform noise at Q 4 (every macroblock 26 - 31 words; the staging fills
    in the middle of a slice of 64 and more; at 33 it stays just under), and "brim" at 33: noise of amplitude 62 or 64 per macroblock
    at Q 2, 33 slots of 28 or 32 words that fill the staging at the last macroblock in some slices and not in others.  Last,
    VECTOR_LEVEL 1 and 2 on the mix clip."""
    cases = []
    for i, mbw in enumerate(WIDTHS):
        for j, content in enumerate(CONTENTS):
            for p, pf in enumerate((0, 3)):
                Q = (1, 2, 4)[(i + j + p) % 3]
                if mbw >= 120 and content == "mix":
                    Q = 2
                if mbw >= 120 and content == "ramp":
                    Q = (2, 1)[(i + p) % 2]
                cases.append((mbw, 8 if content == "ramp" and mbw == 128 else 4, content, 3, Q, pf))
    cases += [(128, 4, "binary", 3, 1, 0), (128, 4, "binary", 3, 1, 3), (128, 8, "ramp", 3, 2, 3)]
    cases += [(33, 4, "noise", 3, 4, 0), (33, 4, "noise", 3, 4, 3), (33, 4, "brim", 3, 2, 0), (33, 4, "brim", 3, 2, 3),
              (64, 4, "noise", 3, 4, 0), (65, 4, "noise", 3, 4, 3), (128, 4, "noise", 3, 4, 0), (128, 4, "noise", 3, 4, 3)]
    cases += [(128, 4, "mix", 1, 2, 3), (128, 4, "mix", 2, 2, 3), (65, 4, "mix", 1, 2, 3), (120, 4, "mix", 2, 1, 3), (127, 4, "mix", 1, 2, 0)]
    return list(dict.fromkeys(cases))


def wide_short_clip(mbw, ys16, content, Q):
    return make_clip(content, 16 * mbw, 16 * ys16, WIDE_SHORT_FRAMES, 1 if content in ("noise", "brim") else 11, Q)


def describe(mb_bits, mbw):
    """mb_bits: the oracle's dump [frames, macroblocks] (bits per macroblock, slice header not included).  -> dict of
       classes      [slices, 4]  macroblocks of every slice in each margined class
       staged_words [slices]     what the slice's <= 990-bit macroblocks take in k_assemble's staging: 16-byte chunks, in words
       slice_bytes  [slices]     38 header bits + the macroblocks, rounded up to bytes
       window_values (3,)        distinct sizes inside each boundary window, over the whole clip
       largest                   the largest macroblock, bits"""
    b = np.asarray(mb_bits).astype(np.int64).reshape(-1, mbw)
    classes = np.stack([((b >= lo) & (b <= hi)).sum(1) for lo, hi in CLASS_BITS], 1)
    words = (b + 31) // 32
    staged = np.where(b <= CLASS_BITS[2][1], (words + 3) // 4 * 4, 0).sum(1)
    return dict(classes=classes, staged_words=staged, slice_bytes=(b.sum(1) + 38 + 7) // 8,
                window_values=tuple(int(np.unique(b[(b >= lo) & (b <= hi)]).size) for lo, hi in WINDOWS), largest=int(b.max()))


def slot_bits(dump, mbw, pframes):
    """The bits k_mb keeps in a macroblock's slot, from the oracle's dump and tables alone: mb_bits less the three codes that need the
    left neighbour and are formed by k_slice_scan / k_assemble instead (csrc/m2v_kernels.hpp mb_dependent): address increment and
    macroblock type (2 bits; 6 for an intra macroblock of a P picture; 4 for an inter one without coefficients) with the motion
    vector differences or the DC differential of the first luma tile, and the DC differentials of U and V.  Predictors come from the
    left neighbour of the same kind inside the slice, else 0 (RTL:2713-2715, 2769-2792).  -> int64 [frames, macroblocks]
    What decides a macroblock's slot class (ceil(slot_bits / 32) words) and what k_assemble's staging counts."""
    L = orc.lib()

    def table(fn, n):
        out = []
        for i in range(n):
            code, ln = ctypes.c_int(0), ctypes.c_int(0)
            fn(i, ctypes.byref(code), ctypes.byref(ln))
            out.append(ln.value)
        return np.array(out, np.int64)
    dc_len = [table(lambda i, c, l, ch=ch: L.m2v_oracle_tab_dc(ch, i, c, l), 12) for ch in (0, 1)]
    mv_len = table(L.m2v_oracle_tab_motion, 17)

    def dc_bits(diff, chroma):
        size = np.where(diff == 0, 0, np.floor(np.log2(np.maximum(np.abs(diff), 1))).astype(np.int64) + 1)
        return dc_len[chroma][size] + size

    def mv_bits(delta):
        d = np.where(delta > 15, delta - 32, np.where(delta < -16, delta + 32, delta))
        return mv_len[np.abs(d)] + (d != 0)
    n = dump["mb_bits"].shape[0]
    shape = (n, -1, mbw)
    inter = dump["mb_inter"].reshape(shape).astype(bool)
    left_inter = np.zeros_like(inter)
    left_inter[:, :, 1:] = inter[:, :, :-1]
    left_intra = np.zeros_like(inter)
    left_intra[:, :, 1:] = ~inter[:, :, :-1]

    def left(a, valid):
        p = np.zeros_like(a)
        p[:, :, 1:] = a[:, :, :-1]
        return np.where(valid, p, 0)
    coef = dump["coef"].astype(np.int64)
    dc = [coef[:, :, t, 0].reshape(shape) for t in range(6)]
    intra_dep = dc_bits(dc[0] - left(dc[3], left_intra), 0) + dc_bits(dc[4] - left(dc[4], left_intra), 1) + dc_bits(dc[5] - left(dc[5], left_intra), 1)
    mvx, mvy = dump["mb_mvx"].reshape(shape).astype(np.int64), dump["mb_mvy"].reshape(shape).astype(np.int64)
    inter_dep = mv_bits(mvx - left(mvx, left_inter)) + mv_bits(mvy - left(mvy, left_inter))
    p_picture = (np.arange(n) % (pframes + 1) != 0)[:, None, None]
    cbp0 = dump["mb_cbp"].reshape(shape) == 0
    dep = np.where(inter, np.where(cbp0, 4, 2) + inter_dep, np.where(p_picture, 6, 2) + intra_dep)
    return (dump["mb_bits"].reshape(shape).astype(np.int64) - dep).reshape(n, -1)


def staged_words_exact(dump, mbw, pframes):
    """per slice: what k_assemble's scan of the compact slots adds up to (16-byte chunks of every macroblock of <= 32 words), and the
    number of macroblocks in the overflow class -> (int64 [slices], int64 [slices])"""
    w = (slot_bits(dump, mbw, pframes).reshape(-1, mbw) + 31) // 32
    return np.where(w <= 32, (w + 3) // 4 * 4, 0).sum(1), (w > 32).sum(1)
