"""Clips for the entropy coder of k_mb (csrc/m2v_kernels.hpp: phase 8 of k_mb - the symbol list, the run/level look-up in
d_ac_code2, the escapes, the bit buffer - and the neighbour-dependent codes of mb_dependent / k_slice_scan / k_assemble), and a
census that says from the oracle's dump alone what a clip reaches.

tests/search_clips.py is for the decision side of k_mb and tests/dense_clips.py for the slot classes and the stream assembly; the
entropy coder was reached by whatever symbols seeded content produces.  The clips here are built coefficient first: target levels
are chosen per tile in zig-zag order, turned into samples by the oracle's own m2v_oracle_dequant and m2v_oracle_idct (on top of
128 for an intra macroblock, on top of the oracle's reconstruction of the picture before for a non-intra one), and encoded; the
census then says what came back.  Conditions (tests/test_entropy_clips.py, CPU) are asserted on what the oracle produced, never
on what was aimed at.

census(clip, xs16, ys16, pframes, VL, Q) restates per macroblock the symbol list as k_mb builds it:
  a non-intra macroblock   [pattern code], then per coded tile [levels ..., end code]; pattern 0: an empty list
  an intra macroblock      Y00 [AC levels ..., end], Y01 / Y10 / Y11 [DC code, AC levels ..., end], U and V [AC ..., end];
                           idxB / idxC are the list indices where U and V begin
Every symbol carries its kind (TABLE / ESCAPE / DC / PATTERN / END), run, level, bank (1 only for the first level of a non-intra
block), list index, length (from the oracle's table accessors) and bit offset inside the macroblock's slot.  The dependent codes
(type, vector deltas, DC of Y00 / U / V) are those of dense_clips.slot_bits.  The anchor of tests/test_entropy_clips.py: the
census's lengths add up to slot_bits on every macroblock, i.e. with the dependent codes to the dump's mb_bits.

The generators (every one returns (clip [n, 3, H, W] uint8, pframes, VL), counts also the recipe of every macroblock):
  intra_codes(Q)      one I picture; every tile's first AC symbol is one target: the 222 signed table codes, the first escape level
                      of every run 0 .. 62, and levels around the clamps of the look-up (40, 41, 42, levels >= 41 at runs >= 32)
  inter_codes(Q)      I P; the I picture is 4 x 4 patches of random luma with flat chroma; every macroblock of the P picture is the
                      reconstruction plus idct(dequant(target)) in its two chroma tiles (chroma takes no part in the decision, so
                      any residual stays inter): every table code as a block's first symbol (bank 1) and behind a +1 at position 0
                      (bank 0), every escape run 0 .. 63 both ways, and the same clamp levels
  intra_zeros(Q), inter_zeros(Q)   the same two with EVERY entry of the rows 0 .. 31 that has no code - 1169 escapes that the look-up
                      must read as 0, not only the first behind each row's codes
  counts(Q)           macroblocks with exact symbol counts (63, 64, 65, 127, 128, 129, the largest there is), intra and non-intra,
                      idxB / idxC at 63 / 64 / 65, escapes at list indices that are multiples of 64, empty and full tiles
  patterns(Q)         every coded block pattern first in a slice and behind an inter neighbour, with and without a vector
  dc_roles(Q)         tiles flat or one step from flat: every DC differential in each role (Y00 against the left neighbour, chained, U, V)
  deltas(VL)          search_clips' displaced-copy macroblocks with neighbours paired for every vector delta
  sizes(Q)            macroblocks whose slot holds exactly 256 / 257 / 512 / 513 / 1024 / 1025 bits

Largest escape the oracle produces from test_gpu_extremes.basis_sign_frames (128 x 96, I + P, VECTOR_LEVEL 3, seed 10 Q + 3), at
Q_LEVEL 1 / 2 / 3 / 4: +-462 / +-254 / +-115 / +-63 (ESCAPE_EXTREMES; tests/test_entropy_clips.py prints and asserts them) - the
escape's 12-bit field is never near its end, and the clips here stay within +-100.
"""
import ctypes
import functools

import numpy as np

import dense_clips as D
import search_clips as S
from oracle import m2v_oracle_ctypes as orc

TABLE, ESCAPE, DC, PATTERN, END = range(5)
ESCAPE_EXTREMES = {1: (-462, 462), 2: (-254, 254), 3: (-115, 115), 4: (-63, 63)}      # Q_LEVEL: (most negative, most positive) escape level
KINDS = ("table", "escape", "dc", "pattern", "end")


# ---------------------------------------------------------------------------------------------------------------------------------
# the oracle's tables and single-stage entry points
# ---------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def tables():
    """-> dict: ac_len [64, 2048] (code length without the sign, 0 = escape), cbp_len [64], dc_len [2][12], zz [64] (zig-zag
    position of raster index), raster [64] (raster index of zig-zag position), table_pairs [(run, level)] of the 111 table codes"""
    L = orc.lib()

    def length(fn, *a):
        c, n = ctypes.c_int(0), ctypes.c_int(0)
        fn(*a, ctypes.byref(c), ctypes.byref(n))
        return n.value
    ac = np.zeros((64, 2048), np.int64)
    for run in range(32):
        for a in range(1, 41):
            ac[run, a] = length(L.m2v_oracle_tab_ac, run, a)
    zz = np.array([L.m2v_oracle_tab_zigzag(i, j) for i in range(8) for j in range(8)], np.int64)
    pairs = [(int(r), int(a)) for r, a in np.argwhere(ac > 0)]
    assert len(pairs) == 111
    return dict(ac_len=ac, cbp_len=np.array([length(L.m2v_oracle_tab_cbp, k) for k in range(64)], np.int64),
                dc_len=[np.array([length(L.m2v_oracle_tab_dc, ch, k) for k in range(12)], np.int64) for ch in (0, 1)],
                zz=zz, raster=np.argsort(zz), table_pairs=pairs)


def last_table_level(run):
    """the largest |level| with a table code at this run; 0 for runs without a row"""
    return int((tables()["ac_len"][run] > 0).sum())


def residual(levels, inter, Q):
    """levels [64] in zig-zag order -> the oracle's idct(dequant(levels)) [8, 8]"""
    L = orc.lib()
    q = np.zeros(64, np.int16)
    q[tables()["raster"]] = np.asarray(levels, np.int16)
    d, r = np.zeros(64, np.int16), np.zeros(64, np.int16)
    L.m2v_oracle_dequant(q.ctypes.data, int(inter), int(Q), d.ctypes.data)
    L.m2v_oracle_idct(d.ctypes.data, r.ctypes.data)
    return r.reshape(8, 8).astype(np.int64)


def dc_size(diff):
    a = np.abs(np.asarray(diff, np.int64))
    return np.where(a == 0, 0, np.floor(np.log2(np.maximum(a, 1))).astype(np.int64) + 1)


def dc_bits(diff, chroma):
    size = dc_size(diff)
    return tables()["dc_len"][chroma][size] + size


# ---------------------------------------------------------------------------------------------------------------------------------
# the census
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_symbols(z, first, bank1):
    """z [64] levels of a tile; first: the position the first run is measured from (-1 non-intra, 0 intra: position 0 is the DC)
    -> list of (kind, run, level, bank, position, length) of the tile's levels and its end code"""
    T = tables()
    out = []
    prev = first
    for p in np.flatnonzero(z):
        p = int(p)
        if p <= first:
            continue
        v, run = int(z[p]), p - prev - 1
        bank = 1 if bank1 and prev == first else 0
        ln = int(T["ac_len"][run, min(abs(v), 2047)])
        if bank and run == 0 and abs(v) == 1:
            out.append((TABLE, run, v, bank, p, 2))            # the '1s' code
        elif ln:
            out.append((TABLE, run, v, bank, p, ln + 1))
        else:
            out.append((ESCAPE, run, v, bank, p, 24))
        prev = p
    out.append((END, 0, 0, 0, 64, 2))
    return out


def mb_symbols(inter, cbp, zig):
    """-> (symbols [(kind, run, level, bank, position, length, tile)], idxB, idxC) of one macroblock as k_mb lists them"""
    T = tables()
    syms, idxB, idxC = [], 0, 0
    if inter:
        if cbp:
            syms.append((PATTERN, 0, cbp, 0, 0, int(T["cbp_len"][cbp]), -1))
            for t in range(6):
                if (cbp >> (5 - t)) & 1:
                    syms += [s + (t,) for s in tile_symbols(zig[t], -1, True)]
    else:
        for t in range(6):
            if t == 4:
                idxB = len(syms)
            if t == 5:
                idxC = len(syms)
            if 1 <= t <= 3:
                diff = int(zig[t][0]) - int(zig[t - 1][0])
                syms.append((DC, 0, diff, 0, 0, int(dc_bits(diff, 0)), t))
            syms += [s + (t,) for s in tile_symbols(zig[t], 0, False)]
    return syms, idxB, idxC


SYM_FIELDS = ("frame", "mb", "intra", "kind", "run", "level", "bank", "position", "length", "tile", "index", "offset", "in_front")


def census(clip, xs16, ys16, pframes, VL, Q, dump=None):
    """-> dict:
       sym      {field: int64 [symbols]} over every symbol of every macroblock, SYM_FIELDS: frame, mb, intra, kind, run, level (a DC
                symbol: the differential; a pattern symbol: the pattern), bank, position (zig-zag), length, tile, index (in the
                macroblock's list), offset (bits from the start of the slot), in_front (the kind of the symbol in front, -1: none)
       per macroblock [frames, mbs]: nsym, idxB, idxC, slot_bits (the census's), inter, cbp, p_picture, first (in its slice),
                left_inter, left_intra, dep (bits of the dependent codes), p1 / p2 / p3 (lengths of the three dependent codes),
                at1 / at2 / at3 (their bit positions in the slice image, the 38-bit slice header included), seg [.., 3]
                (segment lengths A, B, C), seg_at [.., 3], dcd [.., 6] (the DC differential of every tile of an intra macroblock:
                Y00 / U / V against the left intra neighbour or 0), dmv [.., 2] (mv - predictor, not wrapped), pmv [.., 2]
       dump, bytes: the oracle's"""
    clip = np.asarray(clip)
    n = clip.shape[0]
    mbw = xs16
    if dump is None:
        data, d = orc.encode(clip, xs16, ys16, pframes, 7, 7, VL, Q, dump=True)
    else:
        data, d = dump
    mbs = d["mb_bits"].shape[1]
    sym = {k: [] for k in SYM_FIELDS}
    per = {k: np.zeros((n, mbs), np.int64) for k in ("nsym", "idxB", "idxC", "slot_bits")}
    seg = np.zeros((n, mbs, 3), np.int64)
    coef = d["coef"].astype(np.int64)
    for f in range(n):
        for mb in range(mbs):
            inter = int(d["mb_inter"][f, mb])
            syms, idxB, idxC = mb_symbols(inter, int(d["mb_cbp"][f, mb]), coef[f, mb])
            off = 0
            offs = []
            for i, s in enumerate(syms):
                offs.append(off)
                row = (f, mb, 1 - inter, s[0], s[1], s[2], s[3], s[4], s[5], s[6], i, off, syms[i - 1][0] if i else -1)
                for k, v in zip(SYM_FIELDS, row):
                    sym[k].append(v)
                off += s[5]
            offs.append(off)
            per["nsym"][f, mb], per["idxB"][f, mb], per["idxC"][f, mb], per["slot_bits"][f, mb] = len(syms), idxB, idxC, off
            seg[f, mb] = (off, 0, 0) if inter else (offs[idxB], offs[idxC] - offs[idxB], off - offs[idxC])
    out = dict(sym={k: np.array(v, np.int64) for k, v in sym.items()}, dump=d, bytes=data, seg=seg, **per)
    # the dependent codes: their sum from dense_clips.slot_bits, the DC parts from the differentials
    shape = (n, -1, mbw)
    inter = d["mb_inter"].reshape(shape).astype(bool)
    first = np.zeros_like(inter)
    first[:, :, 0] = True
    left_inter, left_intra = np.zeros_like(inter), np.zeros_like(inter)
    left_inter[:, :, 1:], left_intra[:, :, 1:] = inter[:, :, :-1], ~inter[:, :, :-1]

    def left(a, valid):
        p = np.zeros_like(a)
        p[:, :, 1:] = a[:, :, :-1]
        return np.where(valid, p, 0)
    dc = [coef[:, :, t, 0].reshape(shape) for t in range(6)]
    dcd = np.stack([dc[0] - left(dc[3], left_intra), dc[1] - dc[0], dc[2] - dc[1], dc[3] - dc[2],
                    dc[4] - left(dc[4], left_intra), dc[5] - left(dc[5], left_intra)], -1)
    mv = np.stack([d["mb_mvx"].reshape(shape), d["mb_mvy"].reshape(shape)], -1).astype(np.int64)
    pmv = np.stack([left(mv[..., k], left_inter) for k in (0, 1)], -1)
    dep = d["mb_bits"].astype(np.int64) - D.slot_bits(d, mbw, pframes)
    p2 = np.where(inter, 0, dc_bits(dcd[..., 4], 1)).reshape(n, -1)
    p3 = np.where(inter, 0, dc_bits(dcd[..., 5], 1)).reshape(n, -1)
    p1 = dep - p2 - p3
    start = 38 + np.cumsum(d["mb_bits"].astype(np.int64).reshape(shape), -1).reshape(n, -1) - d["mb_bits"]
    at1 = start
    at2 = at1 + p1 + seg[..., 0]
    at3 = at2 + p2 + seg[..., 1]
    out.update(inter=inter.reshape(n, -1), cbp=d["mb_cbp"].astype(np.int64), first=first.reshape(n, -1),
               p_picture=np.broadcast_to((np.arange(n) % (pframes + 1) != 0)[:, None], (n, mbs)),
               left_inter=left_inter.reshape(n, -1), left_intra=left_intra.reshape(n, -1), dep=dep, p1=p1, p2=p2, p3=p3,
               at1=at1, at2=at2, at3=at3, seg_at=np.stack([at1 + p1, at2 + p2, at3 + p3], -1),
               dcd=dcd.reshape(n, -1, 6), dmv=(mv - pmv).reshape(n, -1, 2), pmv=pmv.reshape(n, -1, 2), mv=mv.reshape(n, -1, 2))
    return out


# ---------------------------------------------------------------------------------------------------------------------------------
# construction: levels -> samples
# ---------------------------------------------------------------------------------------------------------------------------------
def tile_of_levels(symbols, dc=0):
    """symbols: [(position, level)] -> [64] zig-zag levels"""
    z = np.zeros(64, np.int64)
    z[0] = dc
    for p, v in symbols:
        z[p] = v
    return z


def paint(frame, by, bx, t, block):
    """put an 8 x 8 block of samples into tile t (Y00, Y01, Y10, Y11, U, V) of macroblock (by, bx) of a 4:4:4 frame [3, H, W];
    a chroma sample is repeated 2 x 2, which the subsampling gives back as it is"""
    block = np.clip(block, 0, 255).astype(np.uint8)
    if t < 4:
        y, x = 16 * by + 8 * (t >> 1), 16 * bx + 8 * (t & 1)
        frame[0, y:y + 8, x:x + 8] = block
    else:
        frame[t - 3, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = np.kron(block, np.ones((2, 2), np.uint8))


def tile_of_recon(recon, W, H, by, bx, t):
    """the 8 x 8 samples of tile t of macroblock (by, bx) in a frame of the dump's `recon` (4:2:0)"""
    if t < 4:
        Y = recon[:W * H].reshape(H, W)
        y, x = 16 * by + 8 * (t >> 1), 16 * bx + 8 * (t & 1)
        return Y[y:y + 8, x:x + 8].astype(np.int64)
    C = recon[W * H + (t - 4) * (W * H // 4):W * H + (t - 3) * (W * H // 4)].reshape(H // 2, W // 2)
    return C[8 * by:8 * by + 8, 8 * bx:8 * bx + 8].astype(np.int64)


def intra_picture(targets, mbh, mbw, Q):
    """targets {(by, bx, t): [64] levels, position 0 the DC level}: 128 + idct(dequant(levels)); every other tile flat 128"""
    f = np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8)
    for (by, bx, t), z in targets.items():
        paint(f, by, bx, t, 128 + residual(z, 0, Q))
    return f


def patch_frame(rng, mbh, mbw):
    """the reference of the non-intra clips: luma 4 x 4 patches of random values 70 .. 185 (no displaced block resembles another, and
    the intra cost is at its cap: a small residual stays inter with the zero vector), chroma flat 128 (it reconstructs exactly)"""
    f = np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8)
    f[0] = np.kron(rng.integers(70, 186, (4 * mbh, 4 * mbw)), np.ones((4, 4), np.int64)).astype(np.uint8)
    return f


def inter_picture(recon, targets, mbh, mbw, Q, vectors=None):
    """the oracle's prediction from the reconstruction `recon` (a frame of the dump) for the vectors [mbh, mbw, 2] (mvx, mvy; None: all
    zero, the reconstruction itself) - search_clips.predicted_frame - plus idct(dequant(levels, inter)) in the tiles of `targets`"""
    H, W = 16 * mbh, 16 * mbw
    f = S.predicted_frame(recon, H, W, np.zeros((mbh, mbw, 2), np.int64) if vectors is None else vectors)
    for (by, bx, t), z in targets.items():
        if t < 4:
            y, x = 16 * by + 8 * (t >> 1), 16 * bx + 8 * (t & 1)
            base = f[0, y:y + 8, x:x + 8].astype(np.int64)
        else:
            base = f[t - 3, 16 * by:16 * by + 16:2, 16 * bx:16 * bx + 16:2].astype(np.int64)
        paint(f, by, bx, t, base + residual(z, 1, Q))
    return f


# ---------------------------------------------------------------------------------------------------------------------------------
# the generators
# ---------------------------------------------------------------------------------------------------------------------------------
Q_LEVELS = (1, 2, 3, 4)
EXTRA_TARGETS = ((0, 40), (0, -40), (0, 41), (0, -41), (0, 42), (0, -42), (1, 40), (5, -100), (40, 30), (33, 45), (33, -45), (36, 60), (36, -60),
                 (32, 41), (32, -41), (62, 41), (62, -41), (5, 100), (5, -99), (45, -70), (50, 55))


def code_targets(last_run):
    """(run, level): the 222 signed table codes, the first escape level of every run 0 .. last_run (the level behind the run's last
    table level; +-1 from run 32 on, the first run without a row), and the levels around the clamps of the look-up"""
    T = tables()
    out = [(r, s * a) for r, a in T["table_pairs"] for s in (1, -1)]
    out += [(r, s * (last_table_level(r) + 1)) for r in range(last_run + 1) for s in (1, -1)]
    out += [(r, v) for r, v in EXTRA_TARGETS if r <= last_run]
    return list(dict.fromkeys(out))


def grid(count, per_mb, mbw=8):
    """-> (mbh, mbw) of a frame that holds `count` targets at per_mb a macroblock, at least 4 rows"""
    return max(4, -(-count // (per_mb * mbw))), mbw


def zero_targets():
    """(run, level): every entry of the rows 0 .. 31 of the look-up that has no code and must read 0 - 32 x 40 less the 111 codes,
    1169 of them - with alternating signs (the look-up takes |level|)"""
    out = [(r, a) for r in range(32) for a in range(last_table_level(r) + 1, 41)]
    return [(r, a if k % 2 else -a) for k, (r, a) in enumerate(out)]


@functools.lru_cache(maxsize=None)
def intra_zeros(Q):
    """intra_codes with zero_targets()"""
    return intra_codes(Q, True)


@functools.lru_cache(maxsize=None)
def inter_zeros(Q):
    """inter_codes with zero_targets()"""
    return inter_codes(Q, True)


@functools.lru_cache(maxsize=None)
def intra_codes(Q, zeros=False):
    """-> (clip, 0, 1): one I picture, one target as the first AC symbol of every tile, all six tiles of a macroblock"""
    todo = zero_targets() if zeros else code_targets(62)
    mbh, mbw = grid(len(todo), 6)
    targets = {}
    for k, (run, v) in enumerate(todo):
        mb, t = divmod(k, 6)
        targets[(mb // mbw, mb % mbw, t)] = tile_of_levels([(run + 1, v)])
    clip = intra_picture(targets, mbh, mbw, Q)[None]
    clip.setflags(write=False)
    return clip, 0, 1


def two_pictures(rng, mbh, mbw, Q, VL, targets, vectors=None):
    """I P: the patch frame and inter_picture(its reconstruction, targets, vectors)"""
    f0 = patch_frame(rng, mbh, mbw)
    _, d = orc.encode(f0[None], mbw, mbh, 0, 7, 7, VL, Q, dump=True)
    clip = np.stack([f0, inter_picture(d["recon"][0], targets, mbh, mbw, Q, vectors)])
    clip.setflags(write=False)
    return clip


@functools.lru_cache(maxsize=None)
def inter_codes(Q, zeros=False):
    """-> (clip, 1, 1).  Every macroblock of the P picture carries one target in U and one in V.  First half of the list: the target
    is the block's first symbol, at zig-zag position `run` (bank 1).  Second half: behind a +1 at position 0, at position run + 1
    (bank 0)."""
    todo = [(0, run, v) for run, v in (zero_targets() if zeros else code_targets(63))] + [(1, run, v) for run, v in (zero_targets() if zeros else code_targets(62))]
    mbh, mbw = grid(len(todo), 2, 16 if zeros else 8)
    targets = {}
    for k, (behind, run, v) in enumerate(todo):
        mb, t = divmod(k, 2)
        targets[(mb // mbw, mb % mbw, 4 + t)] = tile_of_levels([(0, 1), (run + 1, v)] if behind else [(run, v)])
    return two_pictures(np.random.default_rng([Q, 77 + zeros]), mbh, mbw, Q, 1, targets), 1, 1


# ---- exact symbol counts, list indices, empty and full tiles ----
def ones(rng, positions):
    """[(position, +-1)] with seeded signs"""
    return [(int(p), int(rng.choice((-1, 1)))) for p in positions]


def spread(rng, first, count):
    """tiles of `count` levels of +-1 on the positions from `first` up, as many tiles as that takes (63 / 64 positions a tile)"""
    tiles = []
    while count > 0:
        n = min(count, 64 - first)
        tiles.append(ones(rng, range(first, first + n)))
        count -= n
    return tiles


def intra_recipes(rng):
    """{name: six lists of (position, level)}: the AC levels of the six tiles of an intra macroblock.  nsym = 9 + AC levels,
    idxB = 7 + luma AC levels, idxC = idxB + 1 + AC levels of U"""
    E = []                                                # an empty tile
    r = {}
    for nsym in (63, 64, 65, 127, 128, 129, 387):
        t = spread(rng, 1, nsym - 9)
        r["nsym%d" % nsym] = t + [E] * (6 - len(t))
    for idx in (63, 64, 65):
        t = spread(rng, 1, idx - 7)
        r["idxB%d" % idx] = t + [E] * (4 - len(t)) + [ones(rng, (1, 5)), ones(rng, (2,))]
        r["idxC%d" % idx] = [ones(rng, range(1, 21)), E, ones(rng, (3,)), E, ones(rng, range(1, idx - 8 - 21 + 1)), ones(rng, (1, 2, 3))]
    A = lambda n: ones(rng, range(1, n + 1))
    r["escape64_behind_level"] = [A(60), ones(rng, (1, 2, 40)), E, E, E, E]
    r["escape64_behind_dc"] = [A(62), ones(rng, (35,)), E, E, E, E]
    r["escape65_behind_dc64"] = [A(63), ones(rng, (35,)), E, E, E, E]
    r["escape128_behind_dc"] = [A(63), A(61), ones(rng, (40,)), E, E, E]
    r["escape128_behind_level"] = [A(63), A(59), ones(rng, (1, 2, 40)), E, E, E]
    r["escape_behind_end"] = [E, E, E, E, ones(rng, (50,)), ones(rng, (63,))]
    r["escape65_behind_end64"] = [A(57), E, E, E, ones(rng, (1, 2)), ones(rng, (45,))]
    for t in range(6):
        r["empty_tile%d" % t] = [E if k == t else ones(rng, (1, 2 + k, 9)) for k in range(6)]
    r["all_empty"] = [E] * 6
    r["last_at_63"] = [ones(rng, (63,)), ones(rng, (1, 63)), E, ones(rng, (62, 63)), ones(rng, (63,)), ones(rng, (31, 63))]
    return r


def inter_recipes(rng):
    """{name: six lists of (position, level)} of a non-intra macroblock (an empty list: the tile is not coded).
    nsym = 1 + the levels + 1 per coded tile.  Large levels stay in the chroma tiles, which the decision does not see."""
    N = []
    r = {}
    P = lambda n: ones(rng, range(n))
    for nsym, u, v in ((63, 61, 0), (64, 62, 0), (65, 63, 0), (127, 64, 60), (128, 64, 61), (129, 64, 62)):
        r["nsym%d" % nsym] = [N, N, N, N, P(u), P(v)]
    r["nsym391"] = [P(64) for _ in range(6)]
    r["nsym261"] = [N, N] + [P(64) for _ in range(4)]
    r["escape64_behind_end"] = [N, N, N, N, P(62), ones(rng, (40,))]
    r["escape65_behind_end64"] = [N, N, N, N, P(63), ones(rng, (40,))]
    r["escape64_behind_level"] = [N, N, N, N, P(61), ones(rng, (0, 40))]
    r["escape128_behind_level"] = [N, N, N, N, P(64), P(62) + [(63, 19)]]
    r["escape128_behind_end"] = [N, N, N, P(64), P(61), [(33, -2)]]
    r["first_one64"] = [N, N, N, N, P(62), ones(rng, (0, 3))]
    r["first_one128"] = [N, N, N, P(64), P(61), ones(rng, (0, 1))]
    r["first_minus_one_later"] = [N, N, N, N, [(5, 1), (6, -1), (7, 1)], [(0, 2), (1, 1), (2, -1)]]
    r["zero_and_63"] = [N, N, N, N, ones(rng, (0, 63)), ones(rng, (0, 63))]
    r["only_63"] = [N, N, N, N, ones(rng, (63,)), ones(rng, (62, 63))]
    return r


COUNTS_SHAPE = (4, 10)


@functools.lru_cache(maxsize=None)
def counts(Q):
    """-> (clip, 1, 1), three pictures I P I: the patch frame, the non-intra recipes over its reconstruction, the intra recipes.
    Also -> names: {(frame, macroblock): recipe}"""
    rng = np.random.default_rng([Q, 303])
    mbh, mbw = COUNTS_SHAPE
    names, inter_t, intra_t = {}, {}, {}
    for k, (name, tiles) in enumerate(inter_recipes(rng).items()):
        names[(1, k)] = name
        for t, sy in enumerate(tiles):
            if sy:
                inter_t[(k // mbw, k % mbw, t)] = tile_of_levels(sy)
    for k, (name, tiles) in enumerate(intra_recipes(rng).items()):
        names[(2, k)] = name
        for t, sy in enumerate(tiles):
            intra_t[(k // mbw, k % mbw, t)] = tile_of_levels(sy)
    assert max(k for _, k in names) < mbh * mbw
    two = two_pictures(rng, mbh, mbw, Q, 1, inter_t)
    clip = np.concatenate([two, intra_picture(intra_t, mbh, mbw, Q)[None]])
    clip.setflags(write=False)
    return clip, 1, 1, names


# ---- walks: a sequence of values whose successive differences cover a set ----
class Walker:
    """values in [lo, hi]; step(cur) -> the next value, chosen so that next - cur is a difference not made yet (the largest in
    magnitude that fits); when none fits, a move to the end of the range from which the largest one left will fit"""

    def __init__(self, lo, hi, diffs):
        self.lo, self.hi, self.todo = lo, hi, set(diffs)

    def step(self, cur, allowed=lambda v: True):
        fit = [d for d in self.todo if self.lo <= cur + d <= self.hi and allowed(cur + d)]
        if fit:
            d = max(fit, key=lambda d: (abs(d), d))
            self.todo.discard(d)
            return cur + d
        if self.todo:
            d = max(self.todo, key=lambda d: (abs(d), d))
            nxt = self.hi if d < 0 else self.lo
            if allowed(nxt) and nxt != cur:
                self.todo.discard(nxt - cur)
                return nxt
        return cur if allowed(cur) else 0


# ---- DC differentials ----
@functools.lru_cache(maxsize=None)
def dc_levels(Q=2):
    """the intra DC level of a flat tile of every value 0 .. 255, through the oracle: -> int64 [256]; luma tiles give it, and the flat
    chroma tiles (values 4 k + 1 and 4 k + 2 in macroblock k) are asserted to give the same"""
    mbh, mbw = 4, 16
    f = np.zeros((3, 16 * mbh, 16 * mbw), np.uint8)
    v = np.arange(256).reshape(2 * mbh, 2 * mbw)                           # one value a luma tile: 8 x 32 tiles
    f[0] = np.kron(v, np.ones((8, 8), np.int64))
    for k in (1, 2):
        f[k] = np.kron(np.arange(64).reshape(mbh, mbw) * 4 + k, np.ones((16, 16), np.int64))
    _, d = orc.encode(f[None], mbw, mbh, 0, 7, 7, 1, Q, dump=True)
    assert not d["coef"][0, :, :, 1:].any(), "flat tiles have no AC level"
    dc = d["coef"][0, :, :, 0].astype(np.int64).reshape(mbh, mbw, 6)
    lum = np.zeros(256, np.int64)
    for by in range(mbh):
        for bx in range(mbw):
            for t in range(4):
                lum[v[2 * by + (t >> 1), 2 * bx + (t & 1)]] = dc[by, bx, t]
    for k in (1, 2):
        assert np.array_equal(dc[..., 3 + k].reshape(-1), lum[np.arange(64) * 4 + k])
    return lum


DC_SHAPE = (36, 64)
DC_LATTICE = ((0, 0), (1, 1), (0, 1))


def dc_tile(level):
    """8 x 8 samples whose intra DC level is `level`: a flat tile makes a multiple of 4 (the level is the sum of the samples less
    128, over 16); 16 samples one higher - one in each 2 x 2 cell - add 1"""
    t = np.full((8, 8), 128 + (level >> 2), np.int64)
    for y, x in DC_LATTICE[:level & 3]:
        t[y::2, x::2] += 1
    return t


@functools.lru_cache(maxsize=None)
def dc_roles(Q=4):
    """-> (clip, 1, 1): I P.  The I picture: tiles that are flat or one step from flat (dc_tile), whose DC levels walk through every
    differential the level range allows, in each role: Y00 against the left neighbour's Y11, the three chained ones, U, V.  The first
    macroblock of a slice, whose predictors are 0, takes levels of its own.  The P picture: every macroblock the one to its left in the I picture: nothing in the
    reference resembles it, so most are intra again, in a P picture."""
    lv = dc_levels(Q)
    lo, hi = int(lv.min()), int(lv.max())
    diffs, n = range(lo - hi, hi - lo + 1), hi - lo + 1
    wy, wc, wu, wv = (Walker(lo, hi, diffs) for _ in range(4))
    mbh, mbw = DC_SHAPE
    f = np.full((3, 16 * mbh, 16 * mbw), 128, np.uint8)
    for by in range(mbh):
        for bx in range(mbw):
            for t in range(4):
                y = (lo + 37 * by % n if bx == 0 else wy.step(y)) if t == 0 else wc.step(y)
                paint(f, by, bx, t, dc_tile(y))
            u, v = (lo + 53 * by % n, lo + 71 * by % n) if bx == 0 else (wu.step(u), wv.step(v))
            paint(f, by, bx, 4, dc_tile(u))
            paint(f, by, bx, 5, dc_tile(v))
    clip = np.stack([f, np.roll(f, 16, 2)])
    clip.setflags(write=False)
    return clip, 1, 1


# ---- coded block patterns and macroblock types ----
PATTERN_SHAPE = (16, 4)
PATTERN_LUMA, PATTERN_CHROMA = [(1, 2)], [(0, 3), (5, -1)]     # a coded luma tile's levels (small: the decision sees them), a chroma tile's


def noise_macroblock(rng, f, by, bx):
    """binary luma noise, flat chroma of a random value: nothing in the reference predicts it, an intra macroblock of a P picture"""
    f[0, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = rng.choice([10, 245], (16, 16))
    for p in (1, 2):
        f[p, 16 * by:16 * by + 16, 16 * bx:16 * bx + 16] = rng.integers(40, 216)


@functools.lru_cache(maxsize=None)
def patterns(Q):
    """-> (clip, 1, 2): five pairs I P on 4 x 16 macroblocks.  Pairs 0 - 3: macroblock (row r, column c) of pair g aims at pattern
    (16 g + r + 21 c) % 64 - every column holds every pattern once; column 0 is first in its slice, the others follow an inter
    macroblock - and the interior macroblocks carry small vectors.  Pair 4: slices that mix intra macroblocks (noise), inter
    macroblocks without coefficients and coded ones in every order."""
    rng = np.random.default_rng([Q, 505])
    mbh, mbw = PATTERN_SHAPE
    pairs = []
    for g in range(5):
        targets, vectors = {}, np.zeros((mbh, mbw, 2), np.int64)
        kinds = np.full((mbh, mbw), "C")
        if g == 4:
            kinds = np.array([list(("ICNI", "NCIC", "CNNI", "INIC", "NINC", "CICN")[r % 6]) for r in range(mbh)])
        for r in range(mbh):
            for c in range(mbw):
                if 0 < c < mbw - 1 and 0 < r < mbh - 1:
                    vectors[r, c] = ((r + c + g) % 5 - 2, (3 * r + g) % 5 - 2)
                cbp = (16 * g + r + 21 * c) % 64 if g < 4 else (0 if kinds[r, c] == "N" else 1 + (7 * r + c) % 63)
                for t in range(6):
                    if (cbp >> (5 - t)) & 1:
                        targets[(r, c, t)] = tile_of_levels(PATTERN_LUMA if t < 4 else PATTERN_CHROMA)
        two = np.array(two_pictures(rng, mbh, mbw, Q, 2, targets, vectors))
        for r, c in np.argwhere(kinds == "I"):
            noise_macroblock(rng, two[1], r, c)
        pairs.append(two)
    clip = np.concatenate(pairs)
    clip.setflags(write=False)
    return clip, 1, 2


# ---- motion vector deltas ----
DELTA_SHAPE = (6, 16)
DELTA_INTRA_COLUMNS = (5, 11)                            # of the odd rows
DELTA_GOPS = 16                                          # at most
DELTA_Q = 2


def pick(todo, allowed, default=0):
    fit = sorted(v for v in todo if allowed(v))
    if not fit:
        return default
    todo.discard(fit[0])
    return fit[0]


@functools.lru_cache(maxsize=None)
def deltas(VL):
    """-> (clip, 1, VL): pairs I P on 16 x 6 macroblocks.  The I frame is search_clips' texture; every macroblock of the P picture is
    search_clips.predicted_frame's displaced copy of the reconstruction for a vector assigned to it.  Along a slice the two vector
    components walk (Walker) through every delta mv - prev that the range [-4 VL, 4 VL] allows, -8 VL .. 8 VL - past the wrap at
    > 15 and < -16 for VECTOR_LEVEL 3 (and at 16 for 2).  The first macroblock of a slice and the one behind an intra macroblock
    (noise, columns 5 and 11 of the odd rows) take their vector against a predictor of 0 and go through every value that is legal
    there.  Components that point out of the frame are never assigned: the search masks them.  After every pair the oracle says
    what it chose (an odd component next to the frame's border is chosen about every second time, see search_clips), and only that
    is taken off the lists; pairs are added until the lists are empty."""
    R = 4 * VL
    rng = np.random.default_rng([VL, 707])
    mbh, mbw = DELTA_SHAPE
    walk = [Walker(-R, R, range(-2 * R, 2 * R + 1)) for _ in (0, 1)]
    first = [set(range(0, R + 1)), set(range(-R, R + 1))]
    behind = [set(range(-R, R + 1)), set(range(-R, R + 1))]
    pairs = []
    for g in range(DELTA_GOPS):
        left = [set(w.todo) for w in walk] + [set(v) for v in first + behind]
        if not any(left):
            break
        vectors = np.zeros((mbh, mbw, 2), np.int64)
        intra = np.zeros((mbh, mbw), bool)
        intra[1::2][:, list(DELTA_INTRA_COLUMNS)] = True
        for r in range(mbh):
            ok = [lambda v, c=0: True, lambda v, r=r: (v >= 0 or r > 0) and (v <= 0 or r < mbh - 1)]
            cur = [0, 0]
            for c in range(mbw):
                ok[0] = lambda v, c=c: (v >= 0 or c > 0) and (v <= 0 or c < mbw - 1)
                if intra[r, c]:
                    cur = [0, 0]
                    continue
                for k in (0, 1):
                    if c == 0 or intra[r, c - 1]:
                        cur[k] = pick(first[k] if c == 0 else behind[k], ok[k])
                        walk[k].todo.discard(cur[k])
                    else:
                        cur[k] = walk[k].step(cur[k], ok[k])
                vectors[r, c] = cur
        f0 = S.textured_frame(rng, 16 * mbh, 16 * mbw)
        _, d = orc.encode(f0[None], mbw, mbh, 0, 7, 7, VL, DELTA_Q, dump=True)
        p = S.predicted_frame(d["recon"][0], 16 * mbh, 16 * mbw, vectors)
        for r, c in np.argwhere(intra):
            noise_macroblock(rng, p, r, c)
        pairs += [f0, p]
        c = census(np.stack([f0, p]), mbw, mbh, 1, VL, DELTA_Q)
        I = c["inter"]
        for k in (0, 1):
            walk[k].todo = left[k] - set(c["dmv"][I & c["left_inter"]][:, k].tolist())
            first[k] = left[2 + k] - set(c["mv"][I & c["first"]][:, k].tolist())
            behind[k] = left[4 + k] - set(c["mv"][I & c["left_intra"]][:, k].tolist())
    clip = np.stack(pairs)
    clip.setflags(write=False)
    return clip, 1, VL


# ---- exact slot sizes ----
SIZE_BITS = (255, 256, 257, 258, 511, 512, 513, 514, 1023, 1024, 1025, 1026)
SIZES_SHAPE = (4, 8)


def levels_for_bits(rng, bits, base):
    """six tiles of levels of +-1 that take `bits` - `base` bits: a level right behind another (or behind the DC) is '11s', 3 bits, a
    level behind one zero '011s', 4 bits; `base`: the bits of the macroblock without any level"""
    b = next(b for b in range(3) if (bits - base - 4 * b) % 3 == 0)
    a = (bits - base - 4 * b) // 3
    tiles, t, p = [[] for _ in range(6)], 0, 1
    for k in range(a + b):
        p += k < b                                        # the 4-bit ones first: skip a position
        if p > 63:
            t, p = t + 1, 1
        tiles[t].append(p)
        p += 1
    return [ones(rng, q) for q in tiles]


@functools.lru_cache(maxsize=None)
def sizes(Q):
    """-> (clip, 0, 1): one I picture; macroblock k holds levels_for_bits(SIZE_BITS[k]): slots one bit to either side of the class
    boundaries of 8, 16 and 32 words.  An intra macroblock without levels holds 21 bits: three DC codes of size 0, six end codes."""
    rng = np.random.default_rng([Q, 909])
    mbh, mbw = SIZES_SHAPE
    targets = {}
    for k, bits in enumerate(SIZE_BITS):
        for t, sy in enumerate(levels_for_bits(rng, bits, 21)):
            targets[(k // mbw, k % mbw, t)] = tile_of_levels(sy)
    clip = intra_picture(targets, mbh, mbw, Q)[None]
    clip.setflags(write=False)
    return clip, 0, 1


# ---------------------------------------------------------------------------------------------------------------------------------
# the cases: what tests/test_entropy_clips.py asserts its conditions on and tests/test_gpu_entropy.py runs - the same clips
# ---------------------------------------------------------------------------------------------------------------------------------
COUNTS_Q = (1, 2)
PATTERNS_Q = (1, 3)
SIZES_Q = (1, 2)
ZEROS_Q = (1, 2)
DC_Q = 4
GENERATORS = dict(intra_codes=intra_codes, inter_codes=inter_codes, counts=counts, patterns=patterns, dc_roles=dc_roles, deltas=deltas, sizes=sizes,
                  intra_zeros=intra_zeros, inter_zeros=inter_zeros)


def cases():
    """(kind, arg) of every clip; arg is the Q_LEVEL, for "deltas" the VECTOR_LEVEL (Q_LEVEL DELTA_Q)"""
    return ([("intra_codes", Q) for Q in Q_LEVELS] + [("inter_codes", Q) for Q in Q_LEVELS] + [("counts", Q) for Q in COUNTS_Q] +
            [("patterns", Q) for Q in PATTERNS_Q] + [("dc_roles", DC_Q)] + [("deltas", VL) for VL in (1, 2, 3)] + [("sizes", Q) for Q in SIZES_Q] +
            [(kind, Q) for kind in ("intra_zeros", "inter_zeros") for Q in ZEROS_Q])


def case_id(case):
    return "%s-%d" % case


def cached_clip(kind, arg):
    """-> (clip (read-only), pframes, VL, Q)"""
    clip, pf, VL = GENERATORS[kind](arg)[:3]
    return clip, pf, VL, DELTA_Q if kind == "deltas" else arg


def make(kind, arg):
    """-> (clip, pframes, VL, Q); the clip a copy of the generator's (which is cached and read-only)"""
    clip, pf, VL, Q = cached_clip(kind, arg)
    return np.array(clip), pf, VL, Q


@functools.lru_cache(maxsize=None)
def census_of(kind, arg):
    clip, pf, VL, Q = cached_clip(kind, arg)
    return census(clip, clip.shape[3] // 16, clip.shape[2] // 16, pf, VL, Q)
