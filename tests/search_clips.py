"""Clips for the decision side of k_mb (csrc/m2v_kernels.hpp: full-pel search, nine half-pel SADs, the ten-way intra / inter decision,
luma and chroma prediction), and a census that says from the oracle's dump what they reach.

tests/dense_clips.py is for the stream assembly and tests/corner_clips.py for corners of the arithmetic; seeded content leaves a
good part of the search unvisited (of the 81 / 289 / 625 legal vectors of VECTOR_LEVEL 1 / 2 / 3 it chooses 73 / 172 / 449, and
under half of the full-pel candidates ever win a tie).  The clips here visit all of it, so that a fault bound to ONE candidate - a
lane's window offset, a mask at fx == +-YR, the chroma phase of one mv & 3 class, a key that orders two equal SADs the wrong way -
cannot pass:

  all_vectors(VL, Q, seed, klass)   GOPs of I P P.  The I frame is a smooth random texture; every macroblock of a P frame is the
                                    half-pel sample of the oracle's own reconstruction of the frame before it, displaced by a vector
                                    assigned to it: zero residual at that vector, so the oracle chooses it.  klass "interior": a
                                    (8 VL + 1)^2 grid of macroblocks inside a border ring, every legal vector once per P frame.
                                    klass "border": every edge and corner macroblock of a small frame, over as many GOPs as it takes
                                    to give every edge and every corner each vector that is legal there; a single class ("top", "tl",
                                    ...) assigns that class alone.  `seed` permutes the assignment.
  ties(VL, Q, seed)                 a flat plane of 128 with sparse impulses, independent in every frame: SADs are small integers and
                                    candidates tie, full-pel and half-pel
  intra_tie(VL, i, offset)          one macroblock whose intra cost v10[9] equals its smallest half-pel SAD v10[i] exactly
                                    (offset 0), or with v10[i] one unit to either side (offset -1, +1)
  dark_flat(VL)                     flat dark macroblocks on a flat reference: the intra cost under its cap, smaller than, equal to and
                                    larger than every SAD at once
  outward(VL)                       the texture translated by more than the search range out through each side of the frame in
                                    turn: every border macroblock's true match lies on a masked candidate

census(clip, xs16, ys16, pframes, VL, Q, conformant) restates oracle/m2v_oracle.c motion_stage in numpy over the dump's `yuv420` and
`recon`: the full-pel SADs with the sticky 13-bit accumulator, the last-minimum-wins scan, the half-pel grid, the ten values, the
comparison tree.  It is what the conditions of tests/test_search_clips.py (CPU) are computed from, and that module first asserts that
it reproduces the oracle's (mb_inter, mb_mvx, mb_mvy) on every macroblock of every clip here, which is what makes it trustworthy.
Every generator returns (clip [n, 3, H, W] uint8, pframes); tests/test_gpu_search.py (-m gpu) runs them against the oracle.

Measured on the CPU oracle (tests/test_search_clips.py prints them; information, not thresholds):
  ties, both Q_LEVELs and both seeds together, 2800 macroblocks of P pictures per VECTOR_LEVEL:
    VECTOR_LEVEL 1: 939 partial full-pel ties, every one of the 25 candidates a member of at least 150, 24 of them the winner of one
    VECTOR_LEVEL 2: 724 partial ties, every one of the 81 candidates a member of at least 111, 54 the winner of one
    VECTOR_LEVEL 3: 815 partial ties, every one of the 169 candidates a member of at least 99, 79 the winner of one
    (the last candidate scanned wins, so the winners lean to the later ones; tied pairs with dy1 < dy2 and dx1 > dx2: thousands)
  macroblocks in which a pair of half-pel positions ties at the minimum of the nine ("ab:n"), VECTOR_LEVEL 1 / 2 / 3:
    01:646 02:123 03:646 04:723 05:27 06:70 07:32 08:17 12:141 13:638 14:811 15:65 16:53 17:41 18:26 23:99 24:193 25:9 26:18 27:6 28:38
    34:835 35:36 36:95 37:50 38:30 45:92 46:127 47:69 48:49 56:3 57:18 58:5 67:7 68:37 78:2
    01:928 02:58 03:925 04:970 05:30 06:36 07:17 08:6 12:70 13:924 14:1121 15:56 16:22 17:30 18:7 23:35 24:78 25:5 26:5 27:6 28:24
    34:1105 35:39 36:34 37:35 38:8 45:80 46:40 47:56 48:14 56:5 57:8 58:4 67:1 68:19 78:3
    01:1121 02:109 03:1116 04:1140 05:29 06:56 07:22 08:12 12:113 13:1120 14:1273 15:44 16:47 17:40 18:15 23:75 24:112 25:13 26:13 27:9
    28:30 34:1314 35:43 36:64 37:30 38:13 45:53 46:70 47:37 48:26 56:8 57:9 58:10 67:9 68:24 78:7
    (a single (VECTOR_LEVEL, Q_LEVEL, seed) misses up to eight of the 36 pairs; the four clips of a VECTOR_LEVEL together none)
  all_vectors: interior 81 / 289 / 625 of 81 / 289 / 625 vectors in each P picture at Q_LEVEL 1 and 4, seeds 0 and 1; edges and corners
    every legal vector (45 / 153 / 325 per edge, 25 / 81 / 169 per corner) after 90 / 237 / 549 frames at Q_LEVEL 1, 111 / 243 / 597 at 4
"""
import functools

import numpy as np

from oracle import m2v_oracle_ctypes as orc

KLASSES = ("interior", "top", "bottom", "left", "right", "tl", "tr", "bl", "br")
TREE_ORDER = (8, 9, 4, 5, 6, 7, 0, 1, 2, 3)           # find_min_in_10_values: who wins among equal values (RTL:804-840)


# ---------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------
def sad13(col, masked=None):
    """col [..., 16]: the sums of the 16 absolute differences of every pixel column -> {over, diff[11:0]} of the column-serial
    12-bit accumulator with its sticky 13th bit (RTL:1664-1671): once a sum reaches 4096 nothing more is added"""
    c = np.cumsum(col, -1)
    over = c >= 4096
    at = np.take_along_axis(c, over.argmax(-1)[..., None], -1)[..., 0]
    v = np.where(over.any(-1), 4096 | (at & 0xFFF), c[..., -1])
    return v if masked is None else np.where(masked, 4096, v)


def find_min_in_10_values(v):
    """v [..., 10] -> index; the comparison tree of RTL:804-840, vectorised"""
    v = [v[..., k] for k in range(10)]
    lt = [v[2 * k + 1] < v[2 * k] for k in range(5)]
    w = [np.where(lt[k], v[2 * k + 1], v[2 * k]) for k in range(5)]
    x23, x67 = w[1] < w[0], w[3] < w[2]
    lo, hi = np.where(x23, w[1], w[0]), np.where(x67, w[3], w[2])
    i_lo = np.where(x23, 2 + lt[1], 0 + lt[0])
    i_hi = np.where(x67, 6 + lt[3], 4 + lt[2])
    return np.where((w[4] <= lo) & (w[4] <= hi), 8 + lt[4], np.where(lo < hi, i_lo, i_hi))


def half_pel_grid(T, r4):
    """T [N, 18, 18]: the matched block with a border of one sample -> [N, 33, 33], index i + 1 for half-sample row / column i = -1 .. 31
    (RTL:1746-1752).  r4: the rounding of the four-sample mean, 1 (RTL:764) or 2 (ISO, option conformant)."""
    T = T.astype(np.int64)
    a, b, c, d = T[:, :17, :17], T[:, :17, 1:], T[:, 1:, :17], T[:, 1:, 1:]
    h = np.zeros((T.shape[0], 33, 33), np.int64)
    h[:, 1::2, 1::2] = T[:, 1:17, 1:17]
    h[:, 1::2, 0::2] = ((a + b + 1) >> 1)[:, 1:17, :]
    h[:, 0::2, 1::2] = ((a + c + 1) >> 1)[:, :, 1:17]
    h[:, 0::2, 0::2] = (a + b + c + d + r4) >> 2
    return h


def position_classes(mbh, mbw):
    """[mbh, mbw] of indices into KLASSES"""
    by, bx = np.mgrid[0:mbh, 0:mbw]
    t, b, l, r = by == 0, by == mbh - 1, bx == 0, bx == mbw - 1
    k = np.zeros((mbh, mbw), np.int64)
    for name, m in (("top", t), ("bottom", b), ("left", l), ("right", r), ("tl", t & l), ("tr", t & r), ("bl", b & l), ("br", b & r)):
        k[m] = KLASSES.index(name)
    return k


def legal_vectors(klass, VL):
    """the (mvx, mvy) in half samples that a macroblock of the class can carry: [-4 VL, 4 VL] on either axis, and no component that
    points out of the frame through a side the macroblock touches"""
    R = 4 * VL
    xs = range(0 if klass in ("left", "tl", "bl") else -R, (0 if klass in ("right", "tr", "br") else R) + 1)
    ys = range(0 if klass in ("top", "tl", "tr") else -R, (0 if klass in ("bottom", "bl", "br") else R) + 1)
    return [(x, y) for y in ys for x in xs]


def census_frame(cur, ref, VL, r4=1):
    """cur, ref: [P, H, W] (or [H, W]) luma of P pictures and of the reconstructions they are predicted from.  -> dict, per macroblock
    [P, mbh, mbw, ...] (without the P for a single picture):
       cand [C, 2]   (dy, dx) in scan order          sad  [.., C]  the 13-bit SAD of every candidate (masked ones: 4096)
       live [.., C]  not masked and under 4096       tie  [.., C]  live and at the minimum
       fy, fx        the full-pel winner (0, 0 without a live candidate)
       v10  [.., 10] the nine half-pel SADs and the intra cost        idx   what the tree picks
       inter, mvx, mvy                               klass [mbh, mbw]   index into KLASSES"""
    single = np.ndim(cur) == 2
    cur, ref = np.asarray(cur, np.int64).reshape((-1,) + np.shape(cur)[-2:]), np.asarray(ref, np.int64).reshape((-1,) + np.shape(ref)[-2:])
    YR = 2 * VL
    N, H, W = cur.shape
    mbh, mbw = H // 16, W // 16
    P = YR + 1
    refp = np.zeros((N, H + 2 * P, W + 2 * P), np.int64)               # samples outside the frame: 0, as in the oracle (never selected)
    refp[:, P:P + H, P:P + W] = ref
    pic, by, bx = np.mgrid[0:N, 0:mbh, 0:mbw]
    cand = np.array([(dy, dx) for dy in range(-YR, YR + 1) for dx in range(-YR, YR + 1)])
    sad = np.zeros((N, mbh, mbw, len(cand)), np.int64)
    for k, (dy, dx) in enumerate(cand):
        ad = np.abs(cur - refp[:, P + dy:P + dy + H, P + dx:P + dx + W])
        masked = ((bx == 0) & (dx < 0)) | ((bx == mbw - 1) & (dx > 0)) | ((by == 0) & (dy < 0)) | ((by == mbh - 1) & (dy > 0))   # RTL:1642-1645
        sad[..., k] = sad13(ad.reshape(N, mbh, 16, mbw, 16).sum(2), masked)
    live = sad < 4096
    key = np.where(live, sad, 1 << 20)
    tie = live & (sad == key.min(-1)[..., None])
    win = len(cand) - 1 - key[..., ::-1].argmin(-1)                    # among equal minima the last one scanned (RTL:1694-1710)
    have = live.any(-1)
    fy, fx = np.where(have, cand[win, 0], 0), np.where(have, cand[win, 1], 0)
    # the matched block with its border, the half-pel grid, the nine SADs
    yy = (16 * by + fy + P - 1).reshape(-1, 1) + np.arange(18)
    xx = (16 * bx + fx + P - 1).reshape(-1, 1) + np.arange(18)
    hg = half_pel_grid(refp[pic.reshape(-1, 1, 1), yy[:, :, None], xx[:, None, :]], r4)
    blk = cur.reshape(N, mbh, 16, mbw, 16).transpose(0, 1, 3, 2, 4).reshape(-1, 16, 16)
    v10 = np.zeros((blk.shape[0], 10), np.int64)
    fyf, fxf, byf, bxf = fy.reshape(-1), fx.reshape(-1), by.reshape(-1), bx.reshape(-1)
    for hy in (-1, 0, 1):
        for hx in (-1, 0, 1):
            masked = (((bxf == 0) | (fxf == -YR)) & (hx < 0)) | (((bxf == mbw - 1) | (fxf == YR)) & (hx > 0)) | \
                     (((byf == 0) | (fyf == -YR)) & (hy < 0)) | (((byf == mbh - 1) | (fyf == YR)) & (hy > 0))                    # RTL:1757-1760
            ad = np.abs(blk - hg[:, 1 + hy:33 + hy:2, 1 + hx:33 + hx:2])
            v10[:, 3 * (hy + 1) + hx + 1] = sad13(ad.sum(1), masked)
    # the "intra cost": the deviations from the mean accumulate on top of the pixel sum, in 16 bits (RTL:1600, 1774-1777, 1791)
    S = blk.sum((1, 2))
    mean = (S >> 8) & 0xFF
    S = (S + np.abs(blk - mean[:, None, None]).sum((1, 2))) & 0xFFFF
    v10[:, 9] = np.where(S >> 12 == 0, S & 0xFFF, 0xFFF)
    idx = find_min_in_10_values(v10)
    inter = idx != 9
    mvy = np.where(inter, 2 * fyf + idx // 3 - 1, 2 * fyf)
    mvx = np.where(inter, 2 * fxf + idx % 3 - 1, 2 * fxf)
    shape = (N, mbh, mbw)
    out = dict(sad=sad, live=live, tie=tie, fy=fy, fx=fx, v10=v10.reshape(shape + (10,)), idx=idx.reshape(shape),
               inter=inter.reshape(shape), mvx=mvx.reshape(shape), mvy=mvy.reshape(shape))
    if single:
        out = {k: v[0] for k, v in out.items()}
    out.update(cand=cand, klass=position_classes(mbh, mbw))
    return out


def census(clip, xs16, ys16, pframes, VL, Q, conformant=False):
    """The oracle's dump of the clip and census_frame() of the luma of its P pictures against the reconstructions before them.
    -> dict: the fields of census_frame ([P, mbh, mbw, ...]), `frames` (the P pictures' indices), `oracle`: the dump's mb_inter / mb_mvx /
    mb_mvy of the same pictures, [P, mbh, mbw], and `dump`, all of it"""
    clip = np.asarray(clip)
    n, _, H, W = clip.shape
    assert (W, H) == (16 * xs16, 16 * ys16)
    _, d = orc.encode(clip, xs16, ys16, pframes, 7, 7, VL, Q, dump=True, conformant=conformant)
    frames = np.array([f for f in range(n) if f % (pframes + 1)])
    out = census_frame(d["yuv420"][frames, :W * H].reshape(-1, H, W), d["recon"][frames - 1, :W * H].reshape(-1, H, W), VL, 2 if conformant else 1)
    out["frames"] = frames
    out["oracle"] = {k: d[k][frames].reshape(len(frames), ys16, xs16).astype(np.int64) for k in ("mb_inter", "mb_mvx", "mb_mvy")}
    out["dump"] = d
    return out


def census_equals_oracle(c):
    """-> list of (picture, by, bx) where the census's decision or vector is not the oracle's (vectors count on inter macroblocks:
    the dump's are those that were sent)"""
    o = c["oracle"]
    inter = o["mb_inter"] != 0
    bad = (c["inter"] != inter) | (inter & ((c["mvx"] != o["mb_mvx"]) | (c["mvy"] != o["mb_mvy"])))
    return [tuple(int(v) for v in w) for w in np.argwhere(bad)]


def partial_ties(c):
    """the macroblocks whose tie set at the full-pel minimum has at least 2 members and fewer than all live candidates
    -> bool [P, mbh, mbw]"""
    nt, nl = c["tie"].sum(-1), c["live"].sum(-1)
    return (nt >= 2) & (nt < nl)


def half_pel_ties(c):
    """{(a, b): count}, a < b < 9: macroblocks in which the half-pel positions a and b are both unmasked (under 4096) and both at the
    minimum of the nine"""
    v = c["v10"][..., :9].reshape(-1, 9)
    at_min = (v == v.min(-1, keepdims=True)) & (v < 4096)
    return {(a, b): int((at_min[:, a] & at_min[:, b]).sum()) for a in range(9) for b in range(a + 1, 9)}


# ---------------------------------------------------------------------------------------------------------------------------------
# the generators
# ---------------------------------------------------------------------------------------------------------------------------------
def texture(rng, H, W, amp, k):
    """Gaussian noise through a k x k box filter, scaled to a standard deviation of amp / 3 around 128 (so that `amp` is about the
    largest excursion)"""
    g = rng.standard_normal((H + k, W + k))
    s = np.cumsum(np.cumsum(np.pad(g, ((1, 0), (1, 0))), 0), 1)
    box = (s[k:, k:] - s[:-k, k:] - s[k:, :-k] + s[:-k, :-k])[:H, :W] / k
    return np.clip(np.rint(128 + amp / 3.0 * box), 0, 255).astype(np.uint8)


def textured_frame(rng, H, W, amp=32, k=5):
    """[3, H, W]: luma a texture of amplitude amp, chroma the same kind at half the amplitude and half the resolution (every 4:2:0
    sample repeated 2 x 2, which the subsampling gives back as it is)"""
    f = np.zeros((3, H, W), np.uint8)
    f[0] = texture(rng, H, W, amp, k)
    for p in (1, 2):
        f[p] = np.kron(texture(rng, H // 2, W // 2, amp / 2, k), np.ones((2, 2), np.uint8))
    return f


def displaced(plane, y0, x0, size, vy, vx, r4=1):
    """the size x size block of `plane` at (y0, x0) displaced by (vy, vx) half samples: mean2 / mean4 with the RTL's rounding"""
    p = np.pad(plane.astype(np.int64), ((0, 1), (0, 1)))
    y, x = y0 + (vy >> 1), x0 + (vx >> 1)
    assert y >= 0 and x >= 0 and y + size + (vy & 1) <= plane.shape[0] and x + size + (vx & 1) <= plane.shape[1], "the vector leaves the frame"
    a, b = p[y:y + size, x:x + size], p[y:y + size, x + 1:x + size + 1]
    c, d = p[y + 1:y + size + 1, x:x + size], p[y + 1:y + size + 1, x + 1:x + size + 1]
    if vy & 1 and vx & 1:
        return (a + b + c + d + r4) >> 2
    if vx & 1:
        return (a + b + 1) >> 1
    if vy & 1:
        return (a + c + 1) >> 1
    return a


def predicted_frame(recon, H, W, vectors):
    """recon: a frame of the oracle's dump (4:2:0).  vectors [mbh, mbw, 2] (mvx, mvy).  -> [3, H, W]: every macroblock the oracle's own
    prediction for its vector - luma from the half-pel grid, chroma from mv >> 1 - so that its residual there is zero"""
    Y = recon[:W * H].reshape(H, W)
    C = [recon[W * H + p * (W * H // 4):W * H + (p + 1) * (W * H // 4)].reshape(H // 2, W // 2) for p in (0, 1)]
    f = np.zeros((3, H, W), np.uint8)
    for by in range(H // 16):
        for bx in range(W // 16):
            vx, vy = (int(v) for v in vectors[by, bx])
            f[0, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = displaced(Y, 16 * by, 16 * bx, 16, vy, vx)
            for p in (0, 1):
                f[1 + p, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = np.kron(displaced(C[p], 8 * by, 8 * bx, 8, vy >> 1, vx >> 1), np.ones((2, 2), np.int64))
    return f


BORDER_SHAPE = (5, 6)                                    # (mbh, mbw) of the frames of the edge and corner classes
BORDER_ROUNDS = 24


def assigned_classes(klass):
    return KLASSES[:1] if klass == "interior" else KLASSES[1:] if klass == "border" else (klass,)


def vector_maps(rng, mbh, mbw, VL, klass, todo):
    """-> list of [mbh, mbw, 2] vector maps (mvx, mvy), an even number (whole GOPs of I P P).  todo {class: [vectors]}: the
    macroblocks of every assigned class walk through the class's list, neighbours at neighbouring places of it, over as many pictures
    as the class with the fewest macroblocks per vector needs.  The rest of the frame stands still ("interior": the ring) or draws
    legal vectors at random (the edge and corner classes: everything else)."""
    kl = position_classes(mbh, mbw)
    cells = {k: np.argwhere(kl == KLASSES.index(k)) for k in todo}
    npic = max(-(-len(todo[k]) // len(cells[k])) for k in todo)
    npic = max(npic + (npic & 1), 8)                     # (at least 8: a vector that is hard to get is tried several times a round)
    maps = [np.zeros((mbh, mbw, 2), np.int64) for _ in range(npic)]
    if klass != "interior":
        for m in maps:
            for k in KLASSES:
                legal, at = np.array(legal_vectors(k, VL)), kl == KLASSES.index(k)
                m[at] = legal[rng.integers(0, len(legal), int(at.sum()))]
    for k in todo:
        for t, m in enumerate(maps):
            for j, (by, bx) in enumerate(cells[k]):
                m[by, bx] = todo[k][(t * len(cells[k]) + j) % len(todo[k])]
    return maps


def build_gops(VL, Q, f0, maps):
    """f0 [gops, 3, H, W]: the I frames.  -> (clip [3 * gops, 3, H, W], chosen [2 * gops, mbh, mbw, 3]: the oracle's (mb_inter, mb_mvx,
    mb_mvy) of the P pictures).  GOPs of I P P: the first P picture is built from the oracle's reconstruction of the I frame, the
    second from its reconstruction of the first."""
    gops, _, H, W = f0.shape
    assert len(maps) == 2 * gops
    mbh, mbw = H // 16, W // 16
    clip = np.zeros((3 * gops, 3, H, W), np.uint8)
    clip[0::3] = f0
    _, d = orc.encode(f0, mbw, mbh, 0, 7, 7, VL, Q, dump=True)
    for g in range(gops):
        clip[3 * g + 1] = predicted_frame(d["recon"][g], H, W, maps[2 * g])
    clip[2::3] = clip[1::3]                               # placeholders: the reconstruction of picture 1 does not depend on picture 2
    _, d = orc.encode(clip, mbw, mbh, 2, 7, 7, VL, Q, dump=True)
    for g in range(gops):
        clip[3 * g + 2] = predicted_frame(d["recon"][3 * g + 1], H, W, maps[2 * g + 1])
    _, d = orc.encode(clip, mbw, mbh, 2, 7, 7, VL, Q, dump=True)
    p = [f for f in range(3 * gops) if f % 3]
    chosen = np.stack([d[k][p].reshape(len(p), mbh, mbw).astype(np.int64) for k in ("mb_inter", "mb_mvx", "mb_mvy")], -1)
    return clip, chosen


@functools.lru_cache(maxsize=None)
def all_vectors_built(VL, Q, seed=0, klass="interior"):
    """-> (clip, maps [P, mbh, mbw, 2]: the vectors as assigned, mask [mbh, mbw]: the macroblocks of the assigned classes).
    "interior": one GOP, two permutations of all (8 VL + 1)^2 vectors.  The edge and corner classes: a vector with an odd component
    across a side the macroblock touches has ONE way to be chosen - the half-pel position on the outer side of its full-pel
    neighbour is masked (RTL:1757-1760), so the full-pel search has to end on the inner one, which it does for about every second
    such macroblock.  So after the GOPs that give every vector once, the vectors the oracle did not choose are assigned again in
    further GOPs - every GOP on a texture of its own - until every class has had every one of its vectors chosen."""
    rng = np.random.default_rng([seed, VL, KLASSES.index(klass) if klass in KLASSES else 99])
    g = 8 * VL + 1
    mbh, mbw = (g + 2, g + 2) if klass == "interior" else BORDER_SHAPE
    H, W = 16 * mbh, 16 * mbw
    kl = position_classes(mbh, mbw)
    names = assigned_classes(klass)
    if klass == "interior":
        maps = []
        for _ in range(2):
            m = np.zeros((mbh, mbw, 2), np.int64)
            m[1:-1, 1:-1] = rng.permutation(np.array(legal_vectors("interior", VL))).reshape(g, g, 2)
            maps.append(m)
        clip, _ = build_gops(VL, Q, textured_frame(rng, H, W)[None], maps)
    else:
        todo = {k: [tuple(v) for v in rng.permutation(np.array(legal_vectors(k, VL)))] for k in names}
        clips, maps = [], []
        for _ in range(BORDER_ROUNDS):
            more = vector_maps(rng, mbh, mbw, VL, klass, todo)
            c, chosen = build_gops(VL, Q, np.stack([textured_frame(rng, H, W) for _ in range(len(more) // 2)]), more)
            clips.append(c)
            maps += more
            for k in list(todo):
                at = chosen[:, kl == KLASSES.index(k)].reshape(-1, 3)
                got = {(int(x), int(y)) for i, x, y in at if i}
                todo[k] = [v for v in todo[k] if v not in got]
                if not todo[k]:
                    del todo[k]
            if not todo:
                break
        clip = np.concatenate(clips)
    clip.setflags(write=False)
    return clip, np.stack(maps), np.isin(kl, [KLASSES.index(k) for k in names])


def all_vectors(VL, Q, seed=0, klass="interior"):
    """-> (clip, pframes = 2)"""
    return all_vectors_built(VL, Q, seed, klass)[0], 2


TIES_SHAPE = (10, 14)                                     # (mbh, mbw)
TIES_FRAMES = 6                                          # 1 I + 5 P


@functools.lru_cache(maxsize=None)
def ties(VL, Q, seed=0):
    """-> (clip, pframes = 5).  A flat plane of 128; every frame has its own impulses, each macroblock its own density (1/100 .. 1/300)
    and the impulses amplitudes of 6 .. 60 of either sign.  Chroma the same at half resolution."""
    rng = np.random.default_rng([seed, VL, 4242])
    mbh, mbw = TIES_SHAPE
    H, W = 16 * mbh, 16 * mbw

    def plane(h, w, cell):
        dens = np.kron(1.0 / rng.uniform(100, 300, (h // cell, w // cell)), np.ones((cell, cell)))
        hit = rng.random((h, w)) < dens
        a = rng.integers(6, 61, (h, w)) * rng.choice([-1, 1], (h, w))
        return (128 + np.where(hit, a, 0)).astype(np.uint8)
    clip = np.zeros((TIES_FRAMES, 3, H, W), np.uint8)
    for f in range(TIES_FRAMES):
        clip[f, 0] = plane(H, W, 16)
        for p in (1, 2):
            clip[f, p] = np.kron(plane(H // 2, W // 2, 8), np.ones((2, 2), np.uint8))
    clip.setflags(write=False)
    return clip, TIES_FRAMES - 1


# ---- built macroblocks: a flat band of the reference under the macroblock's first rows, a ramp under the rest ----
BUILT_W, BUILT_H, BUILT_BX, BUILT_BY = 64, 80, 1, 2


@functools.lru_cache(maxsize=None)
def built_reference():
    """The I frame of the built clips and its reconstruction's luma.  Rows 24 .. 39 are flat (60, which reconstructs exactly), the rest
    is a ramp of 5 per column and 3 per row.  The built macroblock is (1, 2), rows 32 .. 47: its rows 0 and 1 lie over the flat band for
    every candidate of every VECTOR_LEVEL (rows 25 .. 40 with the half-pel ring), its rows 8 .. 15 over the ramp."""
    W, H = BUILT_W, BUILT_H
    yy, xx = np.mgrid[0:H, 0:W]
    f0 = np.zeros((3, H, W), np.uint8)
    f0[0] = np.where((yy >= 24) & (yy < 40), 60, np.clip(20 + 5 * (xx - 10) + 3 * (yy - 34), 0, 200)).astype(np.uint8)
    f0[1:] = 128
    _, d = orc.encode(f0[None], W // 16, H // 16, 0, 7, 7, 1, 2, dump=True)
    rec = d["recon"][0][:W * H].reshape(H, W).astype(np.int64)
    assert (rec[24:40] == 60).all(), "flat blocks reconstruct exactly"
    f0.setflags(write=False)
    return f0, rec


def built_clip(cur):
    f0, _ = built_reference()
    clip = np.stack([f0, f0])
    clip[1, 0, 16 * BUILT_BY:16 * BUILT_BY + 16, 16 * BUILT_BX:16 * BUILT_BX + 16] = cur.astype(np.uint8)
    clip.setflags(write=False)
    return clip, 1


def built_v10(cur, VL):
    f0, rec = built_reference()
    y = f0[0].astype(np.int64).copy()
    y[16 * BUILT_BY:16 * BUILT_BY + 16, 16 * BUILT_BX:16 * BUILT_BX + 16] = cur
    c = census_frame(y, rec, VL)
    return c["v10"][BUILT_BY, BUILT_BX], (int(c["fy"][BUILT_BY, BUILT_BX]), int(c["fx"][BUILT_BY, BUILT_BX]))


@functools.lru_cache(maxsize=None)
def intra_tie(VL, i, offset=0):
    """-> (clip, pframes = 1), Q_LEVEL 2.  The macroblock is the half-pel sample i of the reconstruction around the origin - exact over
    the ramp, so position i is the best of the nine by a margin - except for pixels of its first two rows lifted to 255: those lie over
    the flat band for every candidate and add the same mass to every full- and half-pel SAD.  The last lifted pixel is then set so
    that v10[i] is exactly 4095 + offset.  The intra cost of a macroblock this bright is 4095 (its 16-bit sum is past 4095:
    RTL:1791), so offset 0 is the tie: position 8 beats the intra cost, the intra cost beats every other position.  For i != 4 no
    full-pel candidate survives (all at 4096 and more), the search stays at the origin and the half-pel stage alone decides."""
    _, rec = built_reference()
    y0, x0 = 16 * BUILT_BY, 16 * BUILT_BX
    cur = displaced(rec, y0, x0, 16, i // 3 - 1, i % 3 - 1).copy()
    target = 4095 + offset
    nl, last = divmod(target, 195)
    flat = cur.reshape(-1)
    assert (flat[:32] == 60).all()
    flat[:nl] = 255
    flat[nl] = 60 + last
    v10, f = built_v10(cur, VL)
    want = target if target < 4096 else 4096 | (v10[i] & 0xFFF)
    others = np.delete(v10[:9], i)
    assert v10[i] == want and (others > max(4095, v10[i])).all() and v10[9] == 4095, (v10, f)
    assert f == (0, 0)
    return built_clip(cur)


OUTWARD_SHAPE = (6, 8)


@functools.lru_cache(maxsize=None)
def outward(VL):
    """-> (clip, pframes = 1): four pairs I P.  The P picture is the I frame's texture translated by 2 VL + 2 samples - more than the
    search range - so that along one side of the frame in turn (left, right, top, bottom) the content comes in from outside: every
    match lies on the far side of that border, on candidates the border macroblocks have masked."""
    mbh, mbw = OUTWARD_SHAPE
    H, W = 16 * mbh, 16 * mbw
    s = 2 * VL + 2
    rng = np.random.default_rng([VL, 99])
    big = np.zeros((3, H + 2 * s, W + 2 * s), np.uint8)
    big[0] = texture(rng, H + 2 * s, W + 2 * s, 32, 5)
    for p in (1, 2):
        big[p] = np.kron(texture(rng, H // 2 + s, W // 2 + s, 16, 5), np.ones((2, 2), np.uint8))
    clip = np.zeros((8, 3, H, W), np.uint8)
    for g, (sy, sx) in enumerate(((0, -s), (0, s), (-s, 0), (s, 0))):      # the P picture shows the texture at this offset: matches at (sy, sx)
        clip[2 * g] = big[:, s:s + H, s:s + W]
        clip[2 * g + 1] = big[:, s + sy:s + sy + H, s + sx:s + sx + W]
    clip.setflags(write=False)
    return clip, 1


DARK_SHAPE = (5, 6)
DARK_REF, DARK_VALUES = 20, (9, 10, 11)


@functools.lru_cache(maxsize=None)
def dark_flat(VL):
    """-> (clip, pframes = 1): three pairs I P of flat frames.  The I frame is 20 everywhere (it reconstructs exactly); every macroblock
    of a P picture is flat 9, 10 or 11, and over the three pairs each macroblock is each of them once.  The one place where the intra
    cost is under its cap of 4095 (a macroblock whose pixel sum is under 4096: RTL:1791) and decides: it is 256 v, every full- and
    half-pel SAD is 256 (20 - v).  v = 9: the intra cost is the smaller one.  v = 10: ALL of them tie - every full-pel candidate, every
    unmasked half-pel position and the intra cost; the last candidate scanned wins the full-pel stage, which masks position 8 (the end
    of the range, or the frame's border), and the intra cost wins the decision against 4, 5, 6, 7, 0 - 3.  v = 11: every SAD ties
    under the intra cost: the vector is twice the last full-pel candidate the position allows, position 4 in front of 0 - 3."""
    mbh, mbw = DARK_SHAPE
    by, bx = np.mgrid[0:mbh, 0:mbw]
    clip = np.full((6, 3, 16 * mbh, 16 * mbw), 128, np.uint8)
    clip[0::2, 0] = DARK_REF
    for g in range(3):
        clip[2 * g + 1, 0] = np.kron(np.array(DARK_VALUES)[(by + bx + g) % 3], np.ones((16, 16), np.int64))
    clip.setflags(write=False)
    return clip, 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases: what tests/test_search_clips.py asserts its conditions on and tests/test_gpu_search.py runs - the same clips
# ---------------------------------------------------------------------------------------------------------------------------------
VECTOR_LEVELS = (1, 2, 3)
Q_LEVELS = (1, 4)
INTERIOR_SEEDS = (0, 1)
TIES_SEEDS = (0, 1)
INTRA_TIE_POSITIONS = (4, 1, 6, 8)                        # the centre, one of 0 - 3, one of 5 - 7, and 8
BUILT_Q = 2                                              # the Q_LEVEL built_reference() was reconstructed with


def cases():
    """(kind, VL, Q, args) of every clip"""
    out = []
    for VL in VECTOR_LEVELS:
        for Q in Q_LEVELS:
            out += [("interior", VL, Q, (seed,)) for seed in INTERIOR_SEEDS]
            out += [("border", VL, Q, (0,))]
            out += [("ties", VL, Q, (seed,)) for seed in TIES_SEEDS]
            out += [("outward", VL, Q, ()), ("dark_flat", VL, Q, ())]
        out += [("intra_tie", VL, BUILT_Q, (i, off)) for i in INTRA_TIE_POSITIONS for off in (-1, 0, 1)]
    return out


def case_id(case):
    kind, VL, Q, args = case
    return "%s-VL%d-Q%d%s" % (kind, VL, Q, "".join("-%d" % a for a in args))


def make(kind, VL, Q, args=()):
    """-> (clip, pframes); the clip a copy of the generator's (which is cached and read-only)"""
    clip, pf = cached_clip(kind, VL, Q, args)
    return np.array(clip), pf


def cached_clip(kind, VL, Q, args=()):
    if kind in ("interior", "border"):
        return all_vectors(VL, Q, args[0], kind)
    if kind == "ties":
        return ties(VL, Q, *args)
    if kind == "intra_tie":
        assert Q == BUILT_Q
        return intra_tie(VL, *args)
    if kind == "outward":
        return outward(VL)
    if kind == "dark_flat":
        return dark_flat(VL)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def census_of(kind, VL, Q, args=(), conformant=False):
    clip, pf = cached_clip(kind, VL, Q, args)
    return census(clip, clip.shape[3] // 16, clip.shape[2] // 16, pf, VL, Q, conformant)


def vectors_crossing(c, rows):
    """c: a census; rows: [(first, last + 1)] macroblock rows of every strip.  -> (set of mvy > 0 carried by inter macroblocks of a
    strip's last row, set of mvy < 0 carried by inter macroblocks of a strip's first row), the frame's own edges left out: the
    vertical components that make a macroblock read the neighbouring strip's rows"""
    inter, mvy = c["oracle"]["mb_inter"] != 0, c["oracle"]["mb_mvy"]
    down, up = set(), set()
    for a, b in rows[:-1]:
        down |= {int(v) for v in mvy[:, b - 1][inter[:, b - 1]] if v > 0}
    for a, b in rows[1:]:
        up |= {int(v) for v in mvy[:, a][inter[:, a]] if v < 0}
    return down, up
