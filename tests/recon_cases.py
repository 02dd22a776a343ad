"""Clips for the reconstructed pictures out (m2v_set_recon_out) and the buffers the encoder must fill for them: shared by
tests/test_recon_cases.py and tests/test_gpu_recon_out.py.  Every expected byte comes from the oracle's `recon` dump - planar I420 of
the coded size, [n, W*H*3/2] - cropped and written out in the layout by the plain numpy below; nothing here looks at what the library
computes."""
import functools

import numpy as np

import fit_cases as F
import gop_cases as G
import scene_cases as SC
import stats_cases as S
from oracle import m2v_oracle_ctypes as orc

M = S.M
LAYOUTS = ("i420", "yv12", "nv12", "nv21")
GUARD = 4096                # bytes behind the last frame that must stay as they were: a page's worth
FILL = 0xA5

# the geometry cases of this feature, in the form of stats_cases.CASES (whose cases "unref", "ionly", "chunks", "conformant" and
# "vl1q4" are used as they are): 5 x 7 macroblocks with 40-byte chroma rows; 18 tiles per tile row
CASES = {
    "g80": dict(W=80, H=112, n=3, pf=2, params=(6, 6, 3, 2), seed=21),
    "g272": dict(W=272, H=64, n=2, pf=1, params=(6, 6, 3, 2), seed=22),
}
# frames of a size that is not whole macroblocks: (w, h) x the kind of the source
FIT_SIZES = ((100, 70), (49, 49))
FIT_KINDS = ("444", "i420", "rgb24")


def write_layout(dump, W, H, layout, region=None):
    """pictures of the oracle's dump [n, W*H*3/2] -> the frames [n, frame bytes] m2v_set_recon_out must write in `layout`: the top-left
    w x h of luma and (w + 1) / 2 x (h + 1) / 2 of each chroma plane (region = (w, h); None: everything), rows without padding"""
    assert layout in LAYOUTS
    w, h = region or (W, H)
    cw, ch = (w + 1) // 2, (h + 1) // 2
    d = np.asarray(dump, np.uint8).reshape(-1, W * H * 3 // 2)
    n = d.shape[0]
    y = d[:, :W * H].reshape(n, H, W)[:, :h, :w]
    u = d[:, W * H:W * H * 5 // 4].reshape(n, H // 2, W // 2)[:, :ch, :cw]
    v = d[:, W * H * 5 // 4:].reshape(n, H // 2, W // 2)[:, :ch, :cw]
    a, b = (u, v) if layout in ("i420", "nv12") else (v, u)
    if layout in ("i420", "yv12"):
        c = np.concatenate([a.reshape(n, -1), b.reshape(n, -1)], axis=1)
    else:
        c = np.stack([a, b], axis=3).reshape(n, -1)
    return np.ascontiguousarray(np.concatenate([y.reshape(n, -1), c], axis=1))


@functools.lru_cache(maxsize=None)
def case(name):
    """-> dict(frames [n, 3, H, W], W, H, n, pf, params, stream, recon [n, W*H*3/2], source (the 4:2:0 pictures as coded))"""
    if name in S.CASES:
        c = dict(S.case(name))
    else:
        c = dict(CASES[name])
        frames = S.clip(c["W"], c["H"], c["n"], c["seed"])
        frames.setflags(write=False)
        stream, dump = orc.encode(frames, c["W"] // 16, c["H"] // 16, c["pf"], *c["params"], dump=True)
        c.update(frames=frames, stream=stream, dump=dump)
    c.update(recon=c["dump"]["recon"], source=c["dump"]["yuv420"], region=None)
    return c


@functools.lru_cache(maxsize=None)
def fit_case(w, h, kind):
    """-> dict(x [n, bytes] source frames of w x h in `kind`, W, H (padded), stream, recon (of the padded pictures), region = (w, h))"""
    c = dict(w=w, h=h, kind=kind, n=3, pf=2, params=(6, 6, 3, 2), seed=11 if w == 100 else 12)
    W, H = F.padded(w, h)
    base = S.clip(W, H, c["n"], c["seed"])[:, :, :h, :w]
    x = S.source_of(np.ascontiguousarray(base), kind, c["seed"])
    stream, dump = orc.encode(F.planes(x, w, h, kind), W // 16, H // 16, c["pf"], *c["params"], dump=True)
    c.update(x=x, W=W, H=H, stream=stream, recon=dump["recon"], source=dump["yuv420"], region=(w, h))
    return c


def _gop_clip(name, pf, Q):
    f, W, H = G.clip_args(name)
    return dict(frames=f, W=W, H=H, n=len(f), pf=pf, params=(6, 6, 3, Q), region=None, source=G.encoded(f, W, H, pf, Q)[1]["yuv420"])


def by_levels(f, W, H, pf, levels):
    """the pictures of a sequence with GOP k at levels[k]: GOPs are closed, so GOP k's are those of the whole clip coded at that level"""
    gop = pf + 1
    return np.concatenate([G.encoded(f, W, H, pf, q)[1]["recon"][k * gop:(k + 1) * gop] for k, q in enumerate(levels)])


@functools.lru_cache(maxsize=None)
def levels_case():
    """m2v_set_gop_levels: "c80", GOPs of 3, 3 and 2 frames at levels 1, 4, 3"""
    c = _gop_clip("c80", 2, 2)
    lv = G.per_gop(G.SCHEDULE, G.ngops(c["n"], c["pf"]))
    c.update(levels=G.SCHEDULE, stream=G.splice(c["frames"], c["W"], c["H"], c["pf"], G.SCHEDULE), recon=by_levels(c["frames"], c["W"], c["H"], c["pf"], lv))
    return c


@functools.lru_cache(maxsize=None)
def cap_case():
    """option "gop_bytes_max" = 3500 on "c80" at Q_LEVEL 1: by the oracle's sizes GOP 0 goes round twice more, GOP 1 once more, GOP 2
    is left alone"""
    g = G.cap_case("b3500")
    c = _gop_clip("c80", g["pf"], g["Q"])
    tries = g["records"]["tries"].tolist()
    assert max(tries) > 1 and min(tries) == 1 and len(set(g["levels"])) > 1, (tries, g["levels"])
    c.update(B=g["B"], levels=g["levels"], stream=g["stream"], recon=by_levels(c["frames"], c["W"], c["H"], c["pf"], g["levels"]))
    return c


@functools.lru_cache(maxsize=None)
def starts_case():
    """m2v_set_gop_starts: "c96", 12 frames, pframes_count 3, GOPs also start at 2 and 7 - the pictures are those of every GOP encoded alone"""
    c = _gop_clip("c96", 3, 2)
    starts = (2, 7)
    f, W, H, pf = c["frames"], c["W"], c["H"], c["pf"]
    gs = SC.gops(c["n"], pf, starts)
    assert [s for s, _ in gs] == [0, 2, 6, 7, 11]
    c.update(starts=starts, stream=SC.expected(f, W, H, pf, starts, Q=2),
             recon=np.concatenate([G.encoded(f[s:s + L], W, H, pf, 2)[1]["recon"] for s, L in gs]))
    return c


def gpu_cases():
    """every expectation tests/test_gpu_recon_out.py compares against, by name"""
    out = {name: case(name) for name in ("unref", "ionly", "chunks", "conformant", "vl1q4", "g80", "g272")}
    out.update({"fit%dx%d_%s" % (w, h, kind): fit_case(w, h, kind) for w, h in FIT_SIZES for kind in FIT_KINDS})
    out.update(levels=levels_case(), cap=cap_case(), starts=starts_case())
    return out
