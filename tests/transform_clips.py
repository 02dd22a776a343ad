"""Clips for the arithmetic of k_mb between the decision and the codes (csrc/m2v_kernels.hpp: 4:4:4 -> 4:2:0, the forward transform on
the matrix cores and on the VALU path, the three quantisers, the two inverse quantisers, the Chen-Wang inverse transform, the final
clip), and a census that says from the oracle's dump alone what a clip reaches.

tests/search_clips.py is for the decision side of k_mb and tests/entropy_clips.py for its entropy coder; the arithmetic in between was
reached by whatever numbers seeded content produces, and a quantiser's decision boundary only by chance.  The clips here are built
residual first: a target is (position i, j, coefficient value C), and solve() searches an 8 x 8 block of legal samples whose transform
has exactly that value at that position - a scaled basis product, then greedy +-1 steps of single samples, each chosen by its exact
contribution D[i][r] D[j][c] to the sum in front of the transform's shift.  Intra tiles sit on top of 128, non-intra tiles on top of the
oracle's reconstruction of the picture before.  Conditions (tests/test_transform_clips.py, CPU) are asserted on what the census finds,
never on what a generator aimed at.

census(clip, pframes, VL, Q, conformant) restates for every tile of every macroblock, from the dump's yuv420 / recon / mb_inter / mb_mvx /
mb_mvy: the prediction (128, or the displaced block of the reconstruction before: search_clips.displaced), the residual, the coefficients
(m2v_oracle_fdct), the levels (m2v_oracle_quant), the inverse quantiser's output (m2v_oracle_dequant), the inverse transform
(m2v_oracle_idct), the sum prediction + idct in front of the final clip, and the reconstruction.  The anchor of
tests/test_transform_clips.py: the levels are the dump's coef and the reconstruction the dump's recon on every macroblock, in both modes.

chain(...) is the same arithmetic in numpy in the FORM the kernel computes it - the first pass of the transform split into three signed
byte limbs, the intra quantiser's division as a multiplication by ceil(2^21 / W), the non-intra quantiser on the signed value with a bias
for negative ones, a numpy Chen-Wang - with single-point faults (FAULTS) that tests/test_transform_clips.py applies one at a time: a
fault the clips cannot see is a missing clip.

The generators (every one returns (clip [n, 3, H, W] uint8, pframes); every clip but "extremes" ends on a picture that repeats the
reconstruction before it - the oracle's at the VECTOR_LEVEL the clip's case runs at (CASE_VL; intra and inter run at all three: an
I picture has no vectors and inter's are all zero at each, asserted, so their reconstruction is the same) - so that the picture with
the targets is referenced and its reconstruction compared directly).  "extremes" is test_gpu_extremes' clip, reused as it is: it reads
the basis from the built library's m2v_debug_table, the one place here that needs the library (tests/test_transform_clips.py asserts
that table equal to the oracle's):
  intra(Q)       I P: the I picture holds, one target a tile, in luma AND in chroma tiles: every AC position at both sides of the level
                 boundaries k = 1, 2, 3 (|C| = (k W << Q) - qoff - 1 and (k W << Q) - qoff), both signs; DC coefficients with every
                 |C| mod 16 of both signs as Y00, as a chained luma tile, as U and as V; flat tiles of 0 and of 255
  intra_max(Q)   I P: every AC position at both sides of the boundary of MAX_LEVEL[Q][position], both signs, luma and chroma
  inter(Q)       I P P: the patch frame of entropy_clips; every macroblock of the first P picture is the reconstruction plus a solved
                 residual in two luma tiles and both chroma tiles: all 64 positions at |C| = (k << (4 + Q)) - 3 and - 2, k = 1, 2, 3,
                 both signs
  intra_p(Q)     I P P: binary noise, then the k = 1 boundaries and the DC residues of intra() - nothing in the reference resembles
                 them, every candidate's SAD is dead and intra wins, in a P picture
  subsample()    I P: chroma tiles whose 2 x 2 cells are all the same (a, b, c, d): the tile's DC level 4 (s - 128) names the sample s
  clipper(Q)     I P P: samples next to 0 and 255, residuals of a few units, a quarter of the P picture's macroblocks new (intra), a
                 quarter with one 4 x 4 patch of luma flipped to the other end of the range (residuals of +-250 that stay non-intra)
  intra_over()    I P P at Q_LEVEL 4: the two recorded blocks OVER_BLOCKS, whose inverse transform leaves -255 .. 255 (and -256 .. 255)
                 downward and upward, in luma and chroma tiles of intra macroblocks of the I picture and of the first P picture
  extremes(Q)    test_gpu_extremes.basis_sign_frames(128, 96, 10 Q + 3) as it is, I P
"""
import functools

import numpy as np

import entropy_clips as E
import search_clips as S
from oracle import m2v_oracle_ctypes as orc

Q_LEVELS = (1, 2, 3, 4)
VECTOR_LEVELS = (1, 2, 3)
# Chen-Wang multipliers of the inverse transform (oracle/m2v_tables.h M2V_W1 .. M2V_W7, the ones of ISO/IEC 13818-4's idct.c; they have
# no accessor: idct_np is asserted equal to m2v_oracle_idct on every tile of every clip, which pins them)
W1, W2, W3, W5, W6, W7 = 2841, 2676, 2408, 1609, 1108, 565


@functools.lru_cache(maxsize=None)
def tables():
    """-> dict: D [8, 8] the transform's basis, W [64] the intra weights in raster order, zz [64] zig-zag position of raster index"""
    L = orc.lib()
    D = np.array([[L.m2v_oracle_tab_dct(i, k) for k in range(8)] for i in range(8)], np.int64)
    W = np.array([L.m2v_oracle_tab_intra_w(i, j) for i in range(8) for j in range(8)], np.int64)
    return dict(D=D, W=W, zz=E.tables()["zz"])


def qoff(W, Q):
    return (W * ((3 << Q) + 2)) >> 3


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's single-stage entries over many tiles
# ---------------------------------------------------------------------------------------------------------------------------------
def _each(name, src, dst, *args):
    fn = getattr(orc.lib(), name)
    a, b, sa, sb = src.ctypes.data, dst.ctypes.data, src.strides[0], dst.strides[0]
    for k in range(src.shape[0]):
        fn(a + k * sa, *args, b + k * sb)
    return dst


class conformant_mode:
    """the oracle's process-global switch around single-stage calls"""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        orc.lib().m2v_oracle_set_conformant(1 if self.on else 0)

    def __exit__(self, *exc):
        orc.lib().m2v_oracle_set_conformant(0)


def o_fdct(x):
    x = np.ascontiguousarray(x, np.int16).reshape(-1, 64)
    return _each("m2v_oracle_fdct", x, np.zeros(x.shape, np.int32)).astype(np.int64)


def _by_kind(name, src, dtype, inter, Q):
    src = np.ascontiguousarray(src, dtype).reshape(-1, 64)
    out = np.zeros(src.shape, np.int16)
    inter = np.broadcast_to(np.asarray(inter, bool), src.shape[:1])
    for kind in (0, 1):
        m = inter == bool(kind)
        if m.any():
            out[m] = _each(name, np.ascontiguousarray(src[m]), np.zeros((int(m.sum()), 64), np.int16), kind, int(Q))
    return out.astype(np.int64)


def o_quant(c, inter, Q):
    return _by_kind("m2v_oracle_quant", c, np.int32, inter, Q)


def o_dequant(q, inter, Q, conformant=False):
    with conformant_mode(conformant):
        return _by_kind("m2v_oracle_dequant", q, np.int16, inter, Q)


def o_idct(d, conformant=False):
    d = np.ascontiguousarray(d, np.int16).reshape(-1, 64)
    with conformant_mode(conformant):
        return _each("m2v_oracle_idct", d, np.zeros(d.shape, np.int16)).astype(np.int64)


def o_subsample(plane):
    H, W = plane.shape
    p, o = np.ascontiguousarray(plane, np.uint8), np.zeros((H // 2, W // 2), np.uint8)
    orc.lib().m2v_oracle_subsample(p.ctypes.data, W, H, o.ctypes.data)
    return o


# ---------------------------------------------------------------------------------------------------------------------------------
# tiles of a 4:2:0 frame
# ---------------------------------------------------------------------------------------------------------------------------------
def to_tiles(planes, H, W):
    """planes [n, W H 3 / 2] (Y, U, V as the dump keeps them) -> int64 [n, mbs, 6, 64]: Y00 Y01 Y10 Y11 U V of every macroblock"""
    planes = np.asarray(planes)
    n, mbh, mbw = planes.shape[0], H // 16, W // 16
    Y = planes[:, :W * H].reshape(n, mbh, 2, 8, mbw, 2, 8).transpose(0, 1, 4, 2, 5, 3, 6).reshape(n, mbh * mbw, 4, 64)
    C = planes[:, W * H:].reshape(n, 2, mbh, 8, mbw, 8).transpose(0, 2, 4, 1, 3, 5).reshape(n, mbh * mbw, 2, 64)
    return np.concatenate([Y, C], 2).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel's form of the arithmetic, in numpy, with single-point faults
# ---------------------------------------------------------------------------------------------------------------------------------
FAULTS = ("recip", "qoff_shift", "inter_bias", "dc_rounding", "dequant_toward_zero", "clip_254", "one_stage_subsampling", "middle_limb")


def subsample_np(p, fault=None):
    """[H, W] -> [H / 2, W / 2]: two stages of (x + y + 1) >> 1, horizontal first (RTL:1086-1089, 1167-1170)"""
    p = np.asarray(p, np.int64)
    a, b, c, d = p[0::2, 0::2], p[0::2, 1::2], p[1::2, 0::2], p[1::2, 1::2]
    if fault == "one_stage_subsampling":
        return (a + b + c + d + 2) >> 2
    return (((c + d + 1) >> 1) + ((a + b + 1) >> 1) + 1) >> 1


def first_pass(x):
    """x [N, 64] residuals -> T [N, 8, 8]: T[r][j] = sum_k x[r][k] D[j][k], the 19-bit first pass (RTL:2029-2036; Z . B16^T of k_mb)"""
    return np.asarray(x, np.int64).reshape(-1, 8, 8) @ tables()["D"].T


def limbs(T, fault=None):
    """the three byte limbs of (T + 0x808080): -> (bytes [3, ...] unsigned, the signed limbs [3, ...] as the matrix cores take them)"""
    e = (T + 0x808080) & 0xFFFFFF
    b = np.stack([(e >> (8 * k)) & 255 for k in range(3)])
    flip = b ^ 0x80
    if fault == "middle_limb":
        flip[1] = b[1]
    return b, np.where(flip >= 128, flip - 256, flip)


def fdct_np(x, mfma, fault=None):
    """x [N, 64] -> C [N, 64]; mfma [N] bool: the tiles whose first pass goes through the limbs"""
    T = first_pass(x)
    _, s = limbs(T, fault)
    T = np.where(np.asarray(mfma, bool)[:, None, None], s[0] + (s[1] << 8) + (s[2] << 16), T)
    t = tables()["D"] @ T
    return ((t + 2048) >> 12).reshape(-1, 64)


def quant_np(C, inter, Q, fault=None, position=None):
    """C [N, 64], inter [N] -> levels [N, 64].  Intra AC: ((|C| + qoff) >> Q) * ceil(2^21 / W) >> 21; DC: (|C| + 8) >> 4; non-intra: on the
    signed value, v = C + 2, plus 2^s - 5 where v is negative, >> s with s = 4 + Q"""
    W = tables()["W"]
    recip = -((-1 << 21) // W)
    if fault == "recip":
        recip = recip.copy()
        recip[position] -= 1
    qo = (W * ((3 << Q) + 2)) >> (2 if fault == "qoff_shift" else 3)
    a = np.abs(C) & 0xFFFF
    intra = ((a + qo) >> Q) * recip >> 21
    intra[:, 0] = a[:, 0] >> 4 if fault == "dc_rounding" else (a[:, 0] + 8) >> 4
    intra = np.sign(C) * intra
    s = 4 + Q
    v = C + 2
    non = (v + np.where(v < 0, (1 << s) - (4 if fault == "inter_bias" else 5), 0)) >> s
    return np.where(np.asarray(inter, bool)[:, None], non, intra)


def dequant_np(q, inter, Q, conformant=False, fault=None, toggled=None):
    """levels [N, 64] -> the inverse quantiser's output (RTL:2129-2150; conformant: ISO/IEC 13818-2 7.4.2.3 - 7.4.4).  toggled: a list
    that receives the mask [N] of the tiles whose coefficient 63 mismatch control toggles"""
    W = tables()["W"]
    inter = np.asarray(inter, bool)[:, None]
    if conformant:
        qs = 2 << Q
        non = (2 * q + np.sign(q)) * 16 * qs
        ac = 2 * q * W * qs
        trunc = lambda t: np.sign(t) * (np.abs(t) // 32)
        d = np.where(inter, trunc(non), trunc(ac))
        d[:, 0] = np.where(inter[:, 0], d[:, 0], 2 * q[:, 0])
        d = np.clip(d, -2048, 2047)
        even = d.sum(1) % 2 == 0
        if toggled is not None:
            toggled.append(even)
        d[:, 63] ^= even.astype(np.int64)
        return d
    non = np.clip((2 * q + np.sign(q)) << Q, -2047, 2047)
    t = q * W
    if Q >= 3:
        t = t << (Q - 3)
    elif fault == "dequant_toward_zero":
        t = np.sign(t) * (np.abs(t) >> (3 - Q))
    else:
        t = t >> (3 - Q)
    ac = np.clip(t, -2047, 2047)
    ac[:, 0] = 2 * q[:, 0]
    return np.where(inter, non, ac)


def idct_np(d, conformant=False, clip=True):
    """d [N, 64] -> [N, 64]: Chen-Wang in wrapping 32-bit arithmetic, the row pass stored in 18 bits (RTL:844-972; conformant: full width
    and the saturation -256 .. 255).  clip = False: what the column pass hands to the clip of RTL:778-783"""
    i32 = np.int32
    a = np.asarray(d).astype(i32).reshape(-1, 8, 8)

    def butterfly(x0, x1, x2, x3, x4, x5, x6, x7, col):
        r = i32(4) if col else i32(0)
        sh = (lambda v: v >> 3) if col else (lambda v: v)
        x8 = i32(W7) * (x4 + x5) + r
        x4 = sh(x8 + i32(W1 - W7) * x4)
        x5 = sh(x8 - i32(W1 + W7) * x5)
        x8 = i32(W3) * (x6 + x7) + r
        x6 = sh(x8 - i32(W3 - W5) * x6)
        x7 = sh(x8 - i32(W3 + W5) * x7)
        x8 = x0 + x1
        x0 = x0 - x1
        x1 = i32(W6) * (x3 + x2) + r
        x2 = sh(x1 - i32(W2 + W6) * x2)
        x3 = sh(x1 + i32(W2 - W6) * x3)
        x1 = x4 + x6
        x4 = x4 - x6
        x6 = x5 + x7
        x5 = x5 - x7
        x7 = x8 + x3
        x8 = x8 - x3
        x3 = x0 + x2
        x0 = x0 - x2
        x2 = (i32(181) * (x4 + x5) + i32(128)) >> 8
        x4 = (i32(181) * (x4 - x5) + i32(128)) >> 8
        return [x7 + x1, x3 + x2, x0 + x4, x8 + x6, x8 - x6, x0 - x4, x3 - x2, x7 - x1]

    with np.errstate(over="ignore"):
        rows = butterfly((a[:, :, 0] << 11) | i32(128), a[:, :, 4] << 11, a[:, :, 6], a[:, :, 2], a[:, :, 1], a[:, :, 7], a[:, :, 5], a[:, :, 3], False)
        rows = np.stack([v >> 8 for v in rows], -1)                     # [N, row, column]
        if not conformant:
            rows = ((rows & 0x3FFFF) ^ 0x20000) - 0x20000                # the 18-bit register
        rows = rows.astype(i32)
        cols = butterfly((rows[:, 0] << 8) + i32(8192), rows[:, 4] << 8, rows[:, 6], rows[:, 2], rows[:, 1], rows[:, 7], rows[:, 5], rows[:, 3], True)
        out = np.stack([v >> 14 for v in cols], 1).astype(np.int64)      # [N, row, column]
    if clip:
        out = np.clip(out, -256 if conformant else -255, 255)
    return out.reshape(-1, 64)


def chain(resid, pred, inter, mfma, Q, conformant=False, fault=None, position=None):
    """the kernel's form from the residual to the reconstruction -> dict: C, lev, deq, idct_raw (in front of the transform's clip), idct,
    presum, recon, toggled (conformant), each [N, 64] ([N])"""
    C = fdct_np(resid, mfma, fault)
    lev = quant_np(C, inter, Q, fault, position)
    tog = []
    deq = dequant_np(lev, inter, Q, conformant, fault, tog)
    raw = idct_np(deq, conformant, clip=False)
    r = np.clip(raw, -256 if conformant else -255, 255)
    toggled = tog[0] if tog else np.zeros(len(lev), bool)
    if conformant:
        skipped = np.asarray(inter, bool) & ~lev.any(1)                 # a block that is not coded is not reconstructed (7.6.8)
        r, raw, toggled = np.where(skipped[:, None], 0, r), np.where(skipped[:, None], 0, raw), toggled & ~skipped
        deq = np.where(skipped[:, None], 0, deq)
    presum = pred + r
    recon = np.clip(presum, 0, 254 if fault == "clip_254" else 255)
    return dict(C=C, lev=lev, deq=deq, idct_raw=raw, idct=r, presum=presum, recon=recon, toggled=toggled)


# ---------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------
def census(clip, pframes, VL, Q, conformant=False):
    """-> dict; per tile [n, mbs, 6, 64] int64 in raster order: cur, pred, resid, C, lev, deq, idct, presum, recon - every one through the
    oracle's single-stage entries; coef (the dump's levels in raster order), rec (the dump's reconstruction); per macroblock [n, mbs]:
    inter; per picture [n]: p_picture; dump, bytes: the oracle's; H, W, Q, conformant"""
    clip = np.asarray(clip)
    n, _, H, W = clip.shape
    mbh, mbw = H // 16, W // 16
    data, d = orc.encode(clip, mbw, mbh, pframes, 7, 7, VL, Q, dump=True, conformant=conformant)
    cur = to_tiles(d["yuv420"], H, W)
    rec = to_tiles(d["recon"], H, W)
    inter = d["mb_inter"].astype(bool)
    pred = np.full(cur.shape, 128, np.int64)
    r4 = 2 if conformant else 1
    for f, mb in np.argwhere(inter):
        by, bx = divmod(int(mb), mbw)
        vx, vy = int(d["mb_mvx"][f, mb]), int(d["mb_mvy"][f, mb])
        ref = d["recon"][f - 1]
        blk = S.displaced(ref[:W * H].reshape(H, W), 16 * by, 16 * bx, 16, vy, vx, r4)
        pred[f, mb, :4] = blk.reshape(2, 8, 2, 8).transpose(0, 2, 1, 3).reshape(4, 64)
        cx, cy = (int(vx / 2), int(vy / 2)) if conformant else (vx >> 1, vy >> 1)     # 7.6.3.7 truncates, the RTL floors (RTL:1854-1888)
        for p in (0, 1):
            plane = ref[W * H + p * (W * H // 4):W * H + (p + 1) * (W * H // 4)].reshape(H // 2, W // 2)
            pred[f, mb, 4 + p] = S.displaced(plane, 8 * by, 8 * bx, 8, cy, cx, r4).reshape(64)
    resid = cur - pred
    tile_inter = np.repeat(inter[:, :, None], 6, 2).reshape(-1)
    C = o_fdct(resid)
    lev = o_quant(C, tile_inter, Q)
    deq = o_dequant(lev, tile_inter, Q, conformant)
    r = o_idct(deq, conformant)
    if conformant:
        skipped = tile_inter & ~lev.any(1)
        deq, r = np.where(skipped[:, None], 0, deq), np.where(skipped[:, None], 0, r)
    shape = cur.shape
    presum = pred + r.reshape(shape)
    out = dict(cur=cur, pred=pred, resid=resid, C=C.reshape(shape), lev=lev.reshape(shape), deq=deq.reshape(shape), idct=r.reshape(shape),
               presum=presum, recon=np.clip(presum, 0, 255), coef=d["coef"].astype(np.int64)[..., tables()["zz"]], rec=rec, inter=inter,
               p_picture=np.arange(n) % (pframes + 1) != 0, dump=d, bytes=data, H=H, W=W, Q=Q, conformant=conformant)
    return out


def chain_of(c, fault=None, position=None):
    """chain() over the tiles of a census (its residuals and predictions); the luma tiles and, in an I picture, the chroma tiles take the
    matrix-core path (kMfmaChroma = kMfmaLuma && !P)"""
    n, mbs = c["inter"].shape
    mfma = np.ones((n, mbs, 6), bool)
    mfma[c["p_picture"], :, 4:] = False
    tile_inter = np.repeat(c["inter"][:, :, None], 6, 2).reshape(-1)
    return chain(c["resid"].reshape(-1, 64), c["pred"].reshape(-1, 64), tile_inter, mfma.reshape(-1), c["Q"], c["conformant"], fault, position)


def select(c, intra=None, chroma=None, p_picture=None):
    """-> bool [n, mbs, 6]: the tiles of intra / non-intra macroblocks, of luma / chroma, of I / P pictures (None: either)"""
    n, mbs = c["inter"].shape
    m = np.ones((n, mbs, 6), bool)
    if intra is not None:
        m &= (c["inter"] != bool(intra))[:, :, None]
    if chroma is not None:
        m &= (np.arange(6) >= 4)[None, None, :] == bool(chroma)
    if p_picture is not None:
        m &= (c["p_picture"] == bool(p_picture))[:, None, None]
    return m


def keys(position, value):
    return np.asarray(position, np.int64) * (1 << 20) + np.asarray(value, np.int64) + (1 << 19)


def reached(c, mask, first=0):
    """-> sorted unique keys(position, C) over the positions first .. 63 of the tiles of `mask`"""
    C = c["C"][mask][:, first:]
    return np.unique(keys(np.arange(first, 64)[None, :], C))


# ---------------------------------------------------------------------------------------------------------------------------------
# the search: a block of legal samples whose transform has a given value at a given position
# ---------------------------------------------------------------------------------------------------------------------------------
def solve(position, want, lo, hi):
    """position [N] raster index 8 i + j, want [N], lo / hi [N, 64] (or scalars): the legal range of every sample of the residual
    -> (x [N, 64] int64, ok [N]: sum P x lies in [4096 want - 2048, 4096 want + 2047], P = outer(D[i], D[j]))"""
    D = tables()["D"]
    position, want = np.asarray(position, np.int64), np.asarray(want, np.int64)
    N = len(position)
    P = (D[position // 8][:, :, None] * D[position % 8][:, None, :]).reshape(N, 64)
    lo, hi = np.broadcast_to(np.asarray(lo, np.int64), (N, 64)), np.broadcast_to(np.asarray(hi, np.int64), (N, 64))
    centre = 4096 * want
    scale = centre / (P * P).sum(1)
    x = np.zeros((N, 64), np.int64)
    for _ in range(24):                                   # the seed: a scaled basis product, scaled again for what the range cut off
        x = np.clip(np.rint(scale[:, None] * P), lo, hi).astype(np.int64)
        t = (P * x).sum(1)
        good = (t != 0) & (np.sign(t) == np.sign(centre))
        scale = np.where(good, scale * centre / np.where(good, t, 1), scale * 1.5)
    big = 1 << 40
    for _ in range(800):
        err = centre - (P * x).sum(1)
        todo = (err > 2048) | (err < -2047)
        if not todo.any():
            break
        up = np.where(x < hi, np.abs(err[:, None] - P), big)
        dn = np.where(x > lo, np.abs(err[:, None] + P), big)
        both = np.concatenate([up, dn], 1)
        k = both.argmin(1)
        move = todo & (both[np.arange(N), k] < np.abs(err))
        if not move.any():
            break
        rows = np.flatnonzero(move)
        x[rows, k[rows] % 64] += np.where(k[rows] < 64, 1, -1)
    err = centre - (P * x).sum(1)
    return x, (err <= 2048) & (err >= -2047)


# ---------------------------------------------------------------------------------------------------------------------------------
# targets
# ---------------------------------------------------------------------------------------------------------------------------------
def intra_boundary(position, k, Q):
    """|C| of the first coefficient that the intra quantiser takes to level k at the position: (k W << Q) - qoff; one less: level k - 1"""
    W = int(tables()["W"][position])
    return ((k * W) << Q) - int(qoff(W, Q))


def intra_ac_targets(Q, ks=(1, 2, 3), levels=None):
    """[(position, C)]: both sides of the boundary of level k (or of levels[position]), both signs, positions 1 .. 63"""
    out = []
    for p in range(1, 64):
        for k in (ks if levels is None else (levels[p],)):
            b = intra_boundary(p, k, Q)
            out += [(p, s * (b - e)) for e in (1, 0) for s in (1, -1)]
    return out


def inter_targets(Q, ks=(1, 2, 3)):
    """[(position, C)]: |C| = (k << (4 + Q)) - 3 (level k - 1) and - 2 (level k), both signs, positions 0 .. 63"""
    return [(p, s * ((k << (4 + Q)) - e)) for p in range(64) for k in ks for e in (3, 2) for s in (1, -1)]


def dc_values():
    """64 DC coefficients: |C| = 16 (3 + r) + r, r = 0 .. 15, both signs - every |C| mod 16 - and one 16 further"""
    return [s * (16 * (3 + r + m) + r) for r in range(16) for s in (1, -1) for m in (0, 1)]


def dc_block(C):
    """[64] samples - 128 whose sum, the DC coefficient (the basis row is 64 s: 64 . 64 = 4096), is C"""
    base, rest = divmod(int(C), 64)
    x = np.full(64, base, np.int64)
    x[(np.arange(rest) * 37) % 64] += 1
    return x


# MAX_LEVEL[Q][position]: the largest level whose boundary solve() reaches from samples - 128 in -128 .. 127, with both signs and on both
# sides; position 0 (the DC) unused.  Measured with max_levels() (tests/test_transform_clips.py asserts the table is what it gives).
MAX_LEVEL = {
    1: (0, 231, 200, 168, 157, 137, 131, 109, 231, 209, 156, 140, 137, 116, 101, 91, 200, 156, 136, 127, 131, 101, 104, 90, 168, 152, 132, 124, 128, 99, 93, 84, 185, 142, 140, 128, 128, 106, 95, 77, 142, 124, 119, 105, 106, 84, 72, 58, 146, 127, 122, 101, 100, 75, 63, 50, 137, 116, 98, 88, 80, 60, 50, 40),
    2: (0, 115, 100, 84, 78, 68, 65, 54, 115, 105, 78, 70, 68, 58, 50, 45, 100, 78, 68, 64, 65, 50, 52, 45, 84, 76, 66, 62, 64, 49, 46, 42, 93, 71, 70, 64, 64, 53, 47, 38, 71, 62, 59, 52, 53, 42, 36, 29, 73, 64, 61, 50, 50, 37, 31, 25, 68, 58, 49, 44, 40, 30, 25, 20),
    3: (0, 58, 50, 42, 39, 34, 33, 27, 58, 52, 39, 35, 34, 29, 25, 23, 50, 39, 34, 32, 33, 25, 26, 23, 42, 38, 33, 31, 32, 25, 23, 21, 46, 35, 35, 32, 32, 26, 24, 19, 35, 31, 30, 26, 26, 21, 18, 14, 36, 32, 30, 25, 25, 19, 16, 12, 34, 29, 24, 22, 20, 15, 12, 10),
    4: (0, 29, 25, 21, 20, 17, 16, 13, 29, 26, 19, 17, 17, 14, 13, 11, 25, 19, 17, 16, 16, 13, 13, 11, 21, 19, 16, 15, 16, 12, 12, 10, 23, 18, 17, 16, 16, 13, 12, 10, 18, 15, 15, 13, 13, 10, 9, 7, 18, 16, 15, 13, 12, 9, 8, 6, 17, 14, 12, 11, 10, 7, 6, 5),
}


def max_levels(Q):
    """-> tuple [64]: per position the largest level k for which solve() finds all four blocks (both sides of the boundary, both signs)"""
    D = tables()["D"]
    out = [0] * 64
    for p in range(1, 64):
        top = int(128 * np.abs(np.outer(D[p // 8], D[p % 8])).sum()) >> 12
        k = int(o_quant(np.eye(64, dtype=np.int64)[p:p + 1] * top, 0, Q)[0, p])
        while k > 0:
            b = intra_boundary(p, k, Q)
            _, ok = solve([p] * 4, [b - 1, 1 - b, b, -b], -128, 127)
            if ok.all():
                break
            k -= 1
        out[p] = k
    return tuple(out)


# ---------------------------------------------------------------------------------------------------------------------------------
# construction
# ---------------------------------------------------------------------------------------------------------------------------------
def place(mbw, y00=(), ych=(), y=(), u=(), v=(), c=(), luma_tiles=lambda mb: (0, 1, 2, 3)):
    """hand the items of the lists to tiles, macroblock after macroblock: y00 only to tile 0, ych to tiles 1 .. 3, y to any luma tile that
    luma_tiles(mb) allows, u / v to tiles 4 / 5, c to either -> (mbh, {(mb, tile): item})"""
    lists = {k: list(val)[::-1] for k, val in dict(y00=y00, ych=ych, y=y, u=u, v=v, c=c).items()}
    out, mb = {}, 0
    while any(lists.values()):
        for t in luma_tiles(mb):
            for name in (("y00", "y") if t == 0 else ("ych", "y")):
                if lists[name]:
                    out[(mb, t)] = lists[name].pop()
                    break
        for t, name in ((4, "u"), (5, "v")):
            for nm in (name, "c"):
                if lists[nm]:
                    out[(mb, t)] = lists[nm].pop()
                    break
        mb += 1
    return max(4, -(-mb // mbw)), out


def solved(slots, base):
    """slots {(mb, tile): (position, C) or a block [64]}; base [mbs, 6, 64]: what the residual sits on -> {(mb, tile): samples [64]};
    a target that solve() misses is left out: the census says what is there"""
    todo = [(k, v) for k, v in slots.items() if isinstance(v, tuple)]
    out = {k: base[k] + np.asarray(v) for k, v in slots.items() if not isinstance(v, tuple)}
    if todo:
        b = np.stack([base[k] for k, _ in todo])
        x, ok = solve([v[0] for _, v in todo], [v[1] for _, v in todo], -b, 255 - b)
        out.update({k: b[n] + x[n] for n, (k, _) in enumerate(todo) if ok[n]})
    return out


def painted(frame, blocks, mbw):
    for (mb, t), blk in blocks.items():
        E.paint(frame, mb // mbw, mb % mbw, t, np.asarray(blk).reshape(8, 8))
    return frame


def with_tail(frames, pframes, Q, VL=1):
    """append the picture that repeats the oracle's reconstruction of the last one (zero vectors): the last picture of `frames` is
    referenced, its reconstruction is needed and compared"""
    frames = np.asarray(frames)
    n, _, H, W = frames.shape
    _, d = orc.encode(frames, W // 16, H // 16, pframes, 7, 7, VL, Q, dump=True)
    tail = S.predicted_frame(d["recon"][n - 1], H, W, np.zeros((H // 16, W // 16, 2), np.int64))
    clip = np.concatenate([frames, tail[None]])
    clip.setflags(write=False)
    return clip


def intra_frame(slots, mbh, mbw):
    base = np.full((mbh * mbw, 6, 64), 128, np.int64)
    return painted(np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8), solved(slots, base), mbw)


def dc_items():
    dc = [dc_block(C) for C in dc_values()]
    flat = [np.full(64, -128, np.int64), np.full(64, 127, np.int64)]
    return dict(y00=dc + flat, ych=dc + flat, u=dc + flat, v=dc + flat)


@functools.lru_cache(maxsize=None)
def intra(Q):
    t = intra_ac_targets(Q)
    mbh, slots = place(32, y=t, c=t, **dc_items())
    return with_tail(intra_frame(slots, mbh, 32)[None], 1, Q), 1


@functools.lru_cache(maxsize=None)
def intra_max(Q):
    t = intra_ac_targets(Q, levels=MAX_LEVEL[Q])
    mbh, slots = place(16, y=t, c=t)
    return with_tail(intra_frame(slots, mbh, 16)[None], 1, Q), 1


def inter_luma_tiles(mb):
    return (0, 3) if mb % 2 == 0 else (1, 2)


@functools.lru_cache(maxsize=None)
def inter(Q):
    """the targets in the first P picture of I P P.  Two luma tiles a macroblock carry a residual, the other two none: their levels are
    all 0 beside coded tiles"""
    t = inter_targets(Q)
    mbw = 32
    mbh, slots = place(mbw, y=t, c=t, luma_tiles=inter_luma_tiles)
    f0 = E.patch_frame(np.random.default_rng([Q, 1201]), mbh, mbw)
    _, d = orc.encode(f0[None], mbw, mbh, 0, 7, 7, 1, Q, dump=True)
    H, W = 16 * mbh, 16 * mbw
    p = S.predicted_frame(d["recon"][0], H, W, np.zeros((mbh, mbw, 2), np.int64))
    painted(p, solved(slots, to_tiles(d["recon"][:1], H, W)[0]), mbw)
    return with_tail(np.stack([f0, p]), 2, Q), 2


@functools.lru_cache(maxsize=None)
def intra_p(Q):
    """I P P: binary noise in luma; then tiles on top of 128 with the k = 1 boundaries and the DC residues"""
    t = intra_ac_targets(Q, ks=(1,))
    mbw = 16
    mbh, slots = place(mbw, y=t, c=t, **dc_items())
    rng = np.random.default_rng([Q, 1303])
    f0 = np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8)
    f0[0] = rng.choice([10, 245], f0[0].shape)
    return with_tail(np.stack([f0, intra_frame(slots, mbh, mbw)]), 2, Q, CASE_VL["intra_p"](Q)), 2


SUBSAMPLE_Q = 2
SUBSAMPLE_CELLS = [(a, b, c, d) for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)] + \
                  [(2, 0, 0, 0), (0, 0, 0, 2), (3, 0, 0, 0), (0, 3, 1, 0), (2, 1, 0, 0), (0, 0, 1, 2), (3, 0, 1, 0), (0, 2, 0, 2), (3, 3, 0, 1), (1, 2, 3, 0)]
SUBSAMPLE_BASES = (0, 101, 252)


@functools.lru_cache(maxsize=None)
def subsample():
    """I P: chroma tile k holds one 2 x 2 cell (a, b / c, d) = base + offsets (at most 255) 64 times; luma flat"""
    cells = [tuple(min(255, base + o) for o in cell) for base in SUBSAMPLE_BASES for cell in SUBSAMPLE_CELLS] + [(255,) * 4, (254, 255, 255, 255), (255, 255, 254, 255)]
    mbw = 8
    mbh = max(4, -(-len(cells) // (2 * mbw)))
    f = np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8)
    for k, cell in enumerate(cells):
        mb, p = divmod(k, 2)
        by, bx = divmod(mb, mbw)
        f[1 + p, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = np.kron(np.ones((8, 8), np.int64), np.array(cell).reshape(2, 2))
    return with_tail(f[None], 1, SUBSAMPLE_Q), 1


CLIPPER_SHAPE = (8, 16)


@functools.lru_cache(maxsize=None)
def clipper(Q):
    """I P P: 4 x 4 patches of samples within 5 of 0 or of 255, in luma and (every 4:2:0 sample repeated 2 x 2) in chroma; the P picture is
    the reconstruction plus residuals of up to 6, but every fourth macroblock is new patches: an intra macroblock in a P picture"""
    rng = np.random.default_rng([Q, 1407])
    mbh, mbw = CLIPPER_SHAPE
    H, W = 16 * mbh, 16 * mbw

    def patches(h, w, k):
        v = rng.integers(0, 6, (h // k, w // k))
        return np.kron(np.where(rng.random(v.shape) < 0.5, v, 255 - v), np.ones((k, k), np.int64)).astype(np.uint8)

    def frame():
        return np.stack([patches(H, W, 4), patches(H, W, 8), patches(H, W, 8)])
    f0, new = frame(), frame()
    _, d = orc.encode(f0[None], mbw, mbh, 0, 7, 7, 1, Q, dump=True)
    rec = S.predicted_frame(d["recon"][0], H, W, np.zeros((mbh, mbw, 2), np.int64))
    p = rec.astype(np.int64)
    p[0] += rng.integers(-6, 7, (H, W))
    for k in (1, 2):
        p[k] += np.kron(rng.integers(-6, 7, (H // 2, W // 2)), np.ones((2, 2), np.int64))
    p = np.clip(p, 0, 255).astype(np.uint8)
    for mb in range(1, mbh * mbw, 4):                   # luma: the reconstruction, but ONE 4 x 4 patch flipped to the other end of the range -
        by, bx = divmod(mb, mbw)                        # 16 residuals of about +-250, a SAD under 4096: still non-intra
        y, x = 16 * by + 4 * (mb % 3), 16 * bx + 4 * (mb % 4)
        p[0, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = rec[0, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16]
        p[0, y:y + 4, x:x + 4] = np.where(rec[0, y:y + 4, x:x + 4] < 128, 255, 0)
    for mb in range(0, mbh * mbw, 4):
        by, bx = divmod(mb, mbw)
        p[:, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = new[:, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16]
    return with_tail(np.stack([f0, p]), 2, Q, CASE_VL["clipper"](Q)), 2


# Two blocks of 8-bit samples whose intra reconstruction at Q_LEVEL 4 overshoots: what the inverse transform's column pass hands to its
# clip (RTL:778-783) is -259 at sample 0 of the first and +257 at sample 0 of the second, in default and in conformant mode.  Found by a
# search over m2v_oracle_fdct / quant / dequant and idct_np: coefficients a little above the level-1 boundary whose sign pulls sample 0
# one way (each comes back a whole step, 0.39 of it too much) and, just below it, with the other sign (each is dropped).  Recorded,
# not searched again; the census says what they do (tests/test_transform_clips.py).
OVER_Q = 4
OVER_BLOCKS = (
    (0, 103, 225, 78, 139, 86, 99, 103, 60, 102, 96, 134, 68, 76, 92, 93, 147, 129, 196, 29, 32, 123, 147, 59, 149, 147, 56, 86, 74, 59, 102, 78,
     142, 56, 117, 30, 100, 125, 79, 134, 42, 82, 111, 123, 55, 69, 98, 131, 73, 84, 113, 89, 126, 88, 159, 17, 159, 100, 92, 97, 46, 170, 108, 104),
    (255, 108, 3, 109, 14, 88, 116, 40, 109, 106, 111, 99, 90, 140, 106, 86, 14, 65, 32, 145, 207, 81, 55, 107, 60, 113, 137, 74, 113, 152, 63, 107,
     61, 208, 83, 123, 63, 66, 94, 88, 100, 98, 109, 46, 181, 140, 122, 62, 67, 87, 64, 144, 68, 173, 59, 156, 63, 88, 124, 80, 97, 7, 139, 93),
)
OVER_SHAPE = (4, 16)
OVER_MBS = ((0, 1), (8, 9))           # the macroblocks that hold the blocks: of the I picture, of the first P picture


@functools.lru_cache(maxsize=None)
def intra_over():
    """I P P on binary noise (as intra_p: nothing predicts a macroblock of the P picture, intra wins).  Macroblocks 0 and 1 of the I picture
    and 8 and 9 of the P picture: tiles Y00 Y01 Y10 Y11 U V hold blocks 0 1 1 0 0 1 of OVER_BLOCKS (the second one of each pair: 1 0 0 1 1 0);
    the rest of the P picture is flat 128"""
    mbh, mbw = OVER_SHAPE
    rng = np.random.default_rng(1509)
    frames = []
    for pic, mbs in enumerate(OVER_MBS):
        f = np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8)
        if pic == 0:
            f[0] = rng.choice([10, 245], f[0].shape)
        for k, mb in enumerate(mbs):
            for t, b in enumerate((0, 1, 1, 0, 0, 1)):
                E.paint(f, mb // mbw, mb % mbw, t, np.array(OVER_BLOCKS[b ^ k]).reshape(8, 8))
        frames.append(f)
    return with_tail(np.stack(frames), 2, OVER_Q, CASE_VL["intra_over"](OVER_Q)), 2


@functools.lru_cache(maxsize=None)
def extremes(Q):
    from test_gpu_extremes import basis_sign_frames
    clip = basis_sign_frames(128, 96, 10 * Q + 3)
    clip.setflags(write=False)
    return clip, 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases: what tests/test_transform_clips.py asserts its conditions on and tests/test_gpu_transform.py runs - the same clips
# ---------------------------------------------------------------------------------------------------------------------------------
GENERATORS = dict(intra=intra, intra_max=intra_max, inter=inter, intra_p=intra_p, subsample=subsample, clipper=clipper, intra_over=intra_over,
                  extremes=extremes)
# the VECTOR_LEVEL of the one case of a kind and Q_LEVEL (intra and inter run at all three)
CASE_VL = dict(intra_max=lambda Q: 1 + Q % 3, intra_p=lambda Q: 1 + (Q + 1) % 3, subsample=lambda Q: 1, clipper=lambda Q: 1 + (Q + 2) % 3,
               intra_over=lambda Q: 2, extremes=lambda Q: 3)
CLIPPER_Q = (1, 2, 3, 4)


def cases():
    """(kind, Q_LEVEL, VECTOR_LEVEL) of every clip.  intra and inter run at every VECTOR_LEVEL: k_mb<VL, P> keeps a lane table of its own
    per instantiation; the clip of a kind and Q_LEVEL is the same at every VECTOR_LEVEL, what the oracle does with it is not"""
    return ([("intra", Q, VL) for Q in Q_LEVELS for VL in VECTOR_LEVELS] + [("inter", Q, VL) for Q in Q_LEVELS for VL in VECTOR_LEVELS] +
            [(kind, Q, CASE_VL[kind](Q)) for kind, levels in (("intra_max", Q_LEVELS), ("intra_p", Q_LEVELS), ("subsample", (SUBSAMPLE_Q,)),
                                                              ("clipper", CLIPPER_Q), ("intra_over", (OVER_Q,)), ("extremes", Q_LEVELS)) for Q in levels])


def case_id(case):
    return "%s-Q%d-VL%d" % case


def cached_clip(kind, Q, VL):
    """-> (clip (read-only), pframes, VL, Q)"""
    clip, pf = GENERATORS[kind]() if kind in ("subsample", "intra_over") else GENERATORS[kind](Q)
    return clip, pf, VL, Q


def make(kind, Q, VL):
    """-> (clip, pframes, VL, Q); the clip a copy of the generator's (which is cached and read-only)"""
    clip, pf, VL, Q = cached_clip(kind, Q, VL)
    return np.array(clip), pf, VL, Q


@functools.lru_cache(maxsize=None)
def census_of(kind, Q, VL, conformant=False):
    clip, pf, VL, Q = cached_clip(kind, Q, VL)
    return census(clip, pf, VL, Q, conformant)
