"""Clips for the picture statistics (option "stats", m2v_picture_stats) and the records the encoder must report for them: shared by
tests/test_stats_cases.py and tests/test_gpu_picture_stats.py.  Every expected value comes from the oracle's dumps (recon, yuv420,
mb_inter, mb_cbp, mb_mvx, mb_mvy, mb_bits); nothing here looks at what the library computes."""
import functools

import numpy as np

import m2v_load
from oracle import m2v_oracle_ctypes as orc

M = m2v_load.load()
DTYPE = M.PICTURE_STAT_DTYPE

# name -> coded size, frames, pframes_count, module parameters (XL, YL, VL, Q), seed.  The sizes are the smallest at which each piece of
# the feature can still go wrong (tests/test_gpu_picture_stats.py says which piece each one is for).
CASES = {
    "unref": dict(W=64, H=64, n=5, pf=2, params=(6, 6, 3, 2), seed=1),
    "ionly": dict(W=64, H=64, n=3, pf=0, params=(6, 6, 3, 2), seed=2),
    "chunks": dict(W=160, H=128, n=7, pf=4, params=(6, 6, 3, 2), seed=3),
    "groups": dict(W=160, H=128, n=7, pf=2, params=(6, 6, 3, 2), seed=4),
    "conformant": dict(W=96, H=64, n=4, pf=3, params=(6, 6, 3, 2), seed=5, conformant=True),
    "port": dict(W=96, H=64, n=5, pf=2, params=(6, 6, 3, 2), seed=6),
    "beats": dict(W=64, H=64, n=3, pf=2, params=(6, 6, 3, 2), seed=7, nbeats=2 * 1024 + 512),      # 2 1/2 frames: the stop cuts the third
}
CASES.update({"vl%dq%d" % (vl, q): dict(W=96, H=64, n=4, pf=3, params=(6, 6, vl, q), seed=8) for vl in (1, 2, 3) for q in (1, 4)})
# frames of a size that is not whole macroblocks (m2v_set_frame_size): source size, input kind (tests/fit_cases.py)
FIT_CASES = {
    "fit444": dict(w=100, h=70, kind="444", n=3, pf=2, params=(6, 6, 3, 2), seed=11),
    "fit420": dict(w=100, h=70, kind="i420", n=3, pf=2, params=(6, 6, 3, 2), seed=11),
    "fitrgb": dict(w=100, h=70, kind="rgb24", n=3, pf=2, params=(6, 6, 3, 2), seed=11),
    "fit49": dict(w=49, h=49, kind="444", n=3, pf=2, params=(6, 6, 3, 2), seed=12),
}


def clip(W, H, n, seed):
    """[n, 3, H, W]: a panning synthetic scene (inter macroblocks with vectors, noise that no quantiser reproduces), and in every odd
    frame a 32 x 32 patch of white noise in all three planes, which the >= 4096 rule of the search turns into intra macroblocks"""
    a = M.synth.clip(W, H, n, clip_index=100 + seed).copy()
    rng = np.random.default_rng(seed)
    for f in range(1, n, 2):
        y, x = 16 * int(rng.integers(0, H // 16 - 1)), 16 * int(rng.integers(0, W // 16 - 1))
        a[f, :, y:y + 32, x:x + 32] = rng.integers(0, 256, (3, 32, 32), dtype=np.uint8)
    return a


def planes420(flat, W, H):
    """one [W*H*3/2] picture of a dump -> Y [H, W], U, V [H/2, W/2]"""
    y, c = W * H, W * H // 4
    return flat[:y].reshape(H, W), flat[y:y + c].reshape(H // 2, W // 2), flat[y + c:].reshape(H // 2, W // 2)


def sse3(src, rec, W, H, region=None):
    """exact squared error of the three planes of one picture over the measured region: region = (w, h) of luma, its chroma
    (w + 1) / 2 x (h + 1) / 2; None = everything"""
    w, h = region or (W, H)
    out = []
    for k, (a, b) in enumerate(zip(planes420(src, W, H), planes420(rec, W, H))):
        rw, rh = (w, h) if k == 0 else ((w + 1) // 2, (h + 1) // 2)
        d = a[:rh, :rw].astype(np.int64) - b[:rh, :rw].astype(np.int64)
        out.append(int((d * d).sum()))
    return out


def samples3(W, H, region=None):
    w, h = region or (W, H)
    c = ((w + 1) // 2) * ((h + 1) // 2)
    return [w * h, c, c]


def records(dump, W, H, pf, region=None):
    """the oracle's dumps of a sequence -> the records m2v_picture_stats must hand out for it"""
    n = dump["recon"].shape[0]
    r = np.zeros(n, DTYPE)
    inter = dump["mb_inter"] != 0
    for f in range(n):
        r[f]["frame"] = f
        r[f]["coding_type"] = 1 if f % (pf + 1) == 0 else 2
        r[f]["sse"] = sse3(dump["yuv420"][f], dump["recon"][f], W, H, region)
        r[f]["mb_bits"] = int(dump["mb_bits"][f].astype(np.int64).sum())
        r[f]["inter_mbs"] = int(inter[f].sum())
        r[f]["intra_mbs"] = int((~inter[f]).sum())
        r[f]["coded_blocks"] = int(np.unpackbits(dump["mb_cbp"][f].astype(np.uint8)).sum())
        r[f]["mv_abs_x"] = int(np.abs(dump["mb_mvx"][f].astype(np.int64))[inter[f]].sum())
        r[f]["mv_abs_y"] = int(np.abs(dump["mb_mvy"][f].astype(np.int64))[inter[f]].sum())
    return r


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(frames [n, 3, H, W], stream, records, dump, + the case's own entries), computed once"""
    c = dict(CASES[name])
    W, H = c["W"], c["H"]
    frames = clip(W, H, c["n"], c["seed"])
    frames.setflags(write=False)
    stream, dump = orc.encode(frames, W // 16, H // 16, c["pf"], *c["params"], nbeats=c.get("nbeats"), dump=True,
                              conformant=c.get("conformant", False))
    c.update(frames=frames, stream=stream, dump=dump, records=records(dump, W, H, c["pf"]))
    return c


@functools.lru_cache(maxsize=None)
def fit_case(name):
    """-> dict(x [n, bytes] source frames of w x h in `kind`, W, H, stream, records (cropped), uncropped (records over all of W x H))"""
    import fit_cases as F
    c = dict(FIT_CASES[name])
    w, h = c["w"], c["h"]
    W, H = F.padded(w, h)
    base = clip(W, H, c["n"], c["seed"])[:, :, :h, :w]           # the planes the source formats are made of (fit_cases.source's recipe)
    x = source_of(np.ascontiguousarray(base), c["kind"], c["seed"])
    planes = F.planes(x, w, h, c["kind"])
    stream, dump = orc.encode(planes, W // 16, H // 16, c["pf"], *c["params"], dump=True)
    c.update(x=x, W=W, H=H, stream=stream, dump=dump, records=records(dump, W, H, c["pf"], (w, h)), uncropped=records(dump, W, H, c["pf"]))
    return c


def source_of(p, kind, seed):
    """three planes [n, 3, h, w] as source frames [n, bytes] of `kind` ("444", "i420" or "rgb24": Y, U, V or R, G, B)"""
    n = p.shape[0]
    if kind == "444":
        return p.reshape(n, -1)
    if kind == "i420":
        return np.ascontiguousarray(np.concatenate([p[:, 0].reshape(n, -1), p[:, 1, ::2, ::2].reshape(n, -1), p[:, 2, ::2, ::2].reshape(n, -1)], axis=1))
    assert kind == "rgb24"
    return np.ascontiguousarray(p.transpose(0, 2, 3, 1)).reshape(n, -1)
