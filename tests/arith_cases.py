"""The arithmetic of the main-syntax decoder at its decision points: the streams it is tried on - shared by tests/test_arith_cases.py
(CPU) and tests/test_gpu_decode_arith.py.  Every case is described once, in this file's own terms (absolute intra DCs, levels by raster
position, vectors per direction), and turned into two things that share nothing else: the stream, written by tests/ilace_writer.py (and
the writers under it; the quant_matrix_extension is tests/ext_writer.py's), and the log tests/arith_ref.py computes the frames from without parsing anything.  Nothing here looks at what
decoder.py, the host build or the device computes: the cases whose content is searched for (a difference of one in a coefficient must
survive the inverse DCT's rounding) are searched with the plain reference and its switches alone.

A picture is dict(type, prec, qst, alt, field, load=(intra, non-intra) matrices a quant_matrix_extension brings, q=slice code or one per row,
rows=[[macroblock, ...], ...]); a macroblock dict(intra=bool, fwd, bwd, motion, dct, quant=code or None, cbp, blocks=[(levels[64] by
raster position, QF[0][0] of an intra block or None)] for the coded blocks in order).

cases() -> name -> dict(stream, log, b, i, x: the options the stream needs, mutants: the switches of arith_ref that must change its
frames, equivalent: the switches that provably cannot, holds: what the builder counted in it).  48 x 32 (3 x 2 macroblocks) unless a
case says why not."""
import functools

import numpy as np

import arith_ref as R
import dec_cases as D
import dec_writer as W
import ext_writer as XW
import ilace_writer as IW
import main_writer as MW

M = D.M

# 6.3.11: the default matrices, raster order (typed from the standard's table)
DEFAULT_INTRA = (8, 16, 19, 22, 26, 27, 29, 34, 16, 16, 22, 24, 27, 29, 34, 37, 19, 22, 26, 27, 29, 34, 34, 38, 22, 22, 26, 27, 29, 34, 37, 40,
                 22, 26, 27, 29, 32, 35, 40, 48, 26, 27, 29, 32, 35, 40, 48, 58, 26, 27, 29, 34, 38, 46, 56, 69, 27, 29, 35, 38, 46, 56, 69, 83)
DEFAULT_NON_INTRA = (16,) * 64
ZIGZAG = tuple(R.zigzag())
ALTERNATE = tuple(sorted(range(64), key=lambda r: MW.ALTERNATE[r >> 3][r & 7]))      # raster index of every scan position


def scan_of(alt):
    return ALTERNATE if alt else ZIGZAG


# ---- one description -> the stream and the log ----
def _writer_block(lv, dc_diff, intra, alt):
    coefs, run = [], 0
    for k, r in enumerate(scan_of(alt)):
        if intra and k == 0:
            assert r == 0
            continue
        if lv[r]:
            coefs.append((run, int(lv[r]), abs(int(lv[r])) > 40))
            run = 0
        else:
            run += 1
    return dict(dc=int(dc_diff), coefs=coefs)


def build(w, h, pictures, seq=None):
    """-> (stream, log)"""
    seq = dict(seq or {})
    field = any(p.get("field") for p in pictures)
    seq.setdefault("progressive", 0 if field else 1)
    mbw, rows = (w + 15) // 16, IW.mb_rows(h, seq["progressive"])
    mats = [tuple(seq.get("intra_matrix") or DEFAULT_INTRA), tuple(seq.get("non_intra_matrix") or DEFAULT_NON_INTRA)]
    wpics, lpics = [], []
    for pic in pictures:
        ptype, prec, qst, alt = pic["type"], pic.get("prec", 2), pic.get("qst", 0), pic.get("alt", 0)
        assert len(pic["rows"]) == rows and all(len(r) == mbw for r in pic["rows"])
        extras = []
        if pic.get("load"):
            extras.append(XW.quant_ext(intra=pic["load"][0], non_intra=pic["load"][1]))
            mats = [tuple(m) if m is not None else mats[k] for k, m in enumerate(pic["load"])]
        slices, lmbs = [], []
        for row, mbs in enumerate(pic["rows"]):
            q = pic["q"][row] if isinstance(pic.get("q", 2), (list, tuple)) else pic.get("q", 2)
            sl, code, pred = dict(q=q, mbs=[]), q, [0, 0, 0]
            for col, mb in enumerate(mbs):
                intra = bool(mb.get("intra"))
                fwd, bwd = (None, None) if intra else (mb.get("fwd"), mb.get("bwd"))
                cbp = 63 if intra else mb.get("cbp", 0)
                if mb.get("quant") is not None:
                    code = mb["quant"]
                if not intra:
                    pred = [1 << (7 + prec)] * 3
                if col == 0:
                    pred = [1 << (7 + prec)] * 3
                blocks, lblocks, src = [], [], iter(mb.get("blocks", ()))
                for b in range(6):
                    if not (cbp >> (5 - b)) & 1:
                        continue
                    lv, dc = next(src)
                    lv = np.asarray(lv, np.int64)
                    comp, diff = (0 if b < 4 else b - 3), 0
                    if intra:
                        diff, pred[comp] = int(dc) - pred[comp], int(dc)
                        assert 0 <= dc < 1 << (8 + prec) and lv[0] == 0
                    else:
                        assert lv.any(), "a coded non-intra block needs a coefficient"
                    blocks.append(_writer_block(lv, diff, intra, alt))
                    lblocks.append((lv[list(scan_of(alt))], diff))
                m = dict(kind="intra" if intra else "pred", quant=mb.get("quant"), blocks=blocks)
                if pic.get("field"):
                    m.update(motion=mb.get("motion", "frame"), dct=mb.get("dct", 0), fwd=fwd, bwd=bwd, cbp=cbp)
                    if ptype == 2 and not intra and fwd is None:
                        m["kind"] = "nomc"
                elif ptype == 3:
                    m.update(fwd=fwd, bwd=bwd, cbp=cbp)
                elif not intra:
                    assert bwd is None and (fwd is not None or cbp)
                    m.update(kind=("coded" if cbp else "not_coded") if fwd is not None else "nomc", cbp=cbp)
                    if fwd is not None:
                        m["mv"] = tuple(fwd)
                sl["mbs"].append(m)
                lmbs.append(dict(row=row, col=col, first=col == 0, intra=intra, fwd=fwd if (fwd is not None or intra or ptype == 3) else (0, 0), bwd=bwd,
                                 motion=mb.get("motion", "frame") if (fwd is not None or bwd is not None) else "frame", nomc=ptype == 2 and not intra and fwd is None,
                                 dct=mb.get("dct", 0) if (intra or cbp) else 0, cbp=cbp, qcode=code, blocks=lblocks))
            slices.append(sl)
        wp = dict(type=ptype, prec=prec, qst=qst, alt=alt, slices=slices, extras=extras)
        if pic.get("field"):
            wp["field"] = True
        if ptype == 3 or pic.get("field"):
            wp["f_code"] = tuple(pic.get("f_code", (1, 1, 1, 1)))
        elif "f_code" in pic:
            wp["f_code"] = tuple(pic["f_code"][:2])
        wpics.append(wp)
        lpics.append(dict(type=ptype, prec=prec, qst=qst, scan=list(scan_of(alt)), matrices=(mats[0], mats[1]), mbs=lmbs, f_code=tuple(pic.get("f_code", (1, 1, 1, 1))),
                          field=bool(pic.get("field"))))
    s, L = IW.stream(w, h, wpics, seq=seq)
    return s, dict(w=w, h=h, mbw=mbw, rows=rows, pictures=lpics, writer=L)


# ---- content ----
def lv(pairs):
    out = np.zeros(64, np.int64)
    for r, v in pairs:
        out[r] = v
    return out


def flat_mb(v, prec=2):
    """an intra macroblock of value v: DC only (mismatch control moves F[7][7] by one: under a quarter of a sample)"""
    return dict(intra=True, blocks=[(lv(()), v << prec)] * 6)


def flat_i(v, mbw=3, mbh=2, **kw):
    return dict(type=1, rows=[[flat_mb(v, kw.get("prec", 2)) for _ in range(mbw)] for _ in range(mbh)], **kw)


def busy_block(rng, intra, prec=2, most=6, level=12):
    pairs = [(int(rng.randint(1 if intra else 0, 24)), int(rng.randint(1, level + 1)) * (1 if rng.randint(2) else -1)) for _ in range(int(rng.randint(2, most + 1)))]
    return (lv(pairs), int(rng.randint(60, 200)) << prec if intra else None)


def busy_i(rng, mbw=3, mbh=2, q=3, **kw):
    """an I picture whose neighbouring samples differ: every residue of a + b and a + b + c + d occurs"""
    mb = lambda: dict(intra=True, dct=int(rng.randint(2)) if kw.get("field") else 0, blocks=[busy_block(rng, True, kw.get("prec", 2)) for _ in range(6)])
    return dict(type=1, q=q, rows=[[mb() for _ in range(mbw)] for _ in range(mbh)], **kw)


def moved(fwd=None, bwd=None, rng=None, cbp=0, **kw):
    m = dict(fwd=fwd, bwd=bwd, cbp=cbp, **kw)
    if cbp:
        m["blocks"] = [busy_block(rng, False, level=9) for _ in range(bin(cbp).count("1"))]
    return m


def samples(c, ctx, mut=()):
    """the final samples of one candidate block under the switches: c = dict(lv=levels by raster, dc=QF[0][0] or None, q=scale code)"""
    scan = scan_of(ctx.get("alt", 0))
    intra = ctx["intra"]
    mats = (ctx["WN"], ctx["WI"]) if "matrices_swapped" in mut else (ctx["WI"], ctx["WN"])
    F = R.coefficients([c["lv"][list(scan)]], scan, [intra], [c["dc"] or 0], [mats[0] if intra else mats[1]],
                       [R.quantiser_scale(c["q"], ctx["qst"], mut)], R.dc_mult(ctx.get("prec", 2), mut), mut)
    pred = (128 if "dc_offset_twice" in mut else 0) if intra else ctx["base"]
    return R._final(pred + R.idct(F, mut)[0], mut), F[0]


def search(seed, gen, ctx, muts, each=2, tries=20000):
    """candidates of gen(rng) until every switch of `muts` changes the samples of `each` of the chosen ones -> the chosen candidates"""
    rng = np.random.RandomState(seed)
    chosen, need = [], {m: each for m in muts}
    for _ in range(tries):
        if not any(need.values()):
            return chosen
        c = gen(rng)
        if c is None:
            continue
        base = samples(c, ctx)[0]
        hit = [m for m in muts if need[m] and not np.array_equal(samples(c, ctx, (m,))[0], base)]
        if hit:
            chosen.append(c)
            for m in hit:
                need[m] -= 1
    raise AssertionError("no input found on which %s decides a sample" % [m for m in need if need[m]])


def ctx_of(intra, qst=0, prec=2, alt=0, base=128, WI=DEFAULT_INTRA, WN=DEFAULT_NON_INTRA):
    return dict(intra=intra, qst=qst, prec=prec, alt=alt, base=base, WI=tuple(WI), WN=tuple(WN))


def pack_pictures(found):
    """[(ctx, [candidates])] -> pictures of 3 x 2 macroblocks: each candidate fills the six blocks of a macroblock that carries its scale
    code as a macroblock quantiser; intra candidates in I pictures, the others in P pictures, each behind a flat I picture of ctx["base"]"""
    pics = []
    for ctx, cands in found:
        params = dict(prec=ctx["prec"], qst=ctx["qst"], alt=ctx["alt"])
        for at in range(0, len(cands), 6):
            six = list(cands[at:at + 6])
            six += [six[-1]] * (6 - len(six))
            mbs = [dict(intra=ctx["intra"], quant=c["q"], fwd=None if ctx["intra"] else (0, 0), cbp=63, blocks=[(c["lv"], c["dc"])] * 6) for c in six]
            if not ctx["intra"]:
                pics.append(flat_i(ctx["base"], **params))
            pics.append(dict(type=1 if ctx["intra"] else 2, q=5, rows=[mbs[:3], mbs[3:]], **params))
    return pics


def pack(found, w=48, h=32, seq=None):
    return build(w, h, pack_pictures(found), seq)


def case(stream_log, mutants=(), b=False, i=False, x=False, equivalent=(), **holds):
    s, log = stream_log
    return dict(stream=s, log=log, b=b, i=i, x=x, mutants=tuple(mutants), equivalent=tuple(equivalent), holds=holds)


# ---- the dequantiser and mismatch control ----
def _gen_negative(intra, codes, qst, W):
    def gen(rng):
        q = int(codes[rng.randint(len(codes))])
        scale = R.quantiser_scale(q, qst)
        pairs = []
        for _ in range(int(rng.randint(3, 12))):
            r, l = int(rng.randint(1, 64)), -int(rng.randint(1, 12 if intra else 30))
            if ((2 * l - (0 if intra else 1)) * W[r] * scale) % 32:
                pairs.append((r, l))
        return dict(lv=lv(pairs), dc=int(rng.randint(300, 700)) if intra else None, q=q, tag="neg") if pairs else None
    return gen


@functools.lru_cache(maxsize=None)
def trunc_intra():
    ctx = ctx_of(True)
    return case(pack([(ctx, search(1, _gen_negative(True, range(1, 9), 0, DEFAULT_INTRA), ctx, ("dq_floor",), each=6))]), ("dq_floor",))


@functools.lru_cache(maxsize=None)
def trunc_non_intra():
    ctx = ctx_of(False, qst=1)
    return case(pack([(ctx, search(2, _gen_negative(False, (1, 3, 5, 7), 1, DEFAULT_NON_INTRA), ctx, ("dq_floor",), each=6))]), ("dq_floor",))


@functools.lru_cache(maxsize=None)
def sign_term():
    ctx = ctx_of(False, qst=1)

    def gen(rng):
        pairs = [(int(rng.randint(0, 64)), int(rng.randint(1, 30)) * (1 if rng.randint(2) else -1)) for _ in range(int(rng.randint(3, 12)))]
        return dict(lv=lv(pairs), dc=None, q=int((1, 3, 5, 7, 2, 9)[rng.randint(6)]))
    return case(pack([(ctx, search(3, gen, ctx, ("sign_dropped", "sign_plus1"), each=3))]), ("sign_dropped", "sign_plus1"))


W_1_255_I = tuple([8] + [1 if (r + (r >> 3)) & 1 else 255 for r in range(1, 64)])
W_1_255_N = tuple(255 if (r + (r >> 3)) & 1 else 1 for r in range(64))


def _weights_found():
    found, largest = [], 0
    for intra in (True, False):
        for qst, codes in ((0, (31,)), (1, (1, 31))):
            ctx = ctx_of(intra, qst=qst, WI=W_1_255_I, WN=W_1_255_N)

            def gen(rng, intra=intra, codes=codes):
                pairs = [(int(rng.randint(1 if intra else 0, 64)), int((2047, -2047, 2047, -2047, 1, -1, 100, -100)[rng.randint(8)])) for _ in range(int(rng.randint(1, 5)))]
                return dict(lv=lv(pairs), dc=512 if intra else None, q=int(codes[rng.randint(len(codes))]))
            got = search(4 + qst + 2 * intra, gen, ctx, ("prod16", "prod24"), each=3)
            for c in got:
                W_ = W_1_255_I if intra else W_1_255_N
                largest = max(largest, max(abs((2 * int(l) + (0 if intra else int(np.sign(l)))) * W_[r] * R.quantiser_scale(c["q"], qst)) for r, l in enumerate(c["lv"])))
            found.append((ctx, got))
    return found, largest


@functools.lru_cache(maxsize=None)
def weights_1_255():
    """weights 1 and 255 in both matrices (sequence header), levels +-2047, scales 62 (type 0, code 31), 1 and 112 (type 1, codes 1, 31)"""
    found, largest = _weights_found()
    return case(pack(found, seq=dict(intra_matrix=list(W_1_255_I), non_intra_matrix=list(W_1_255_N))), ("prod16", "prod24"), largest=largest)


@functools.lru_cache(maxsize=None)
def weights_1_255_qme():
    """the same pictures with the matrices brought by a quant_matrix_extension behind the first picture's coding extension"""
    found, largest = _weights_found()
    pics = pack_pictures(found)
    pics[0]["load"] = (list(W_1_255_I), list(W_1_255_N))
    return case(build(48, 32, pics), ("prod16", "prod24"), x=True, largest=largest)


@functools.lru_cache(maxsize=None)
def scale_codes():
    """32 x 496: 31 slices of two macroblocks; in each picture slice k carries code k and its second macroblock code 32 - k as a
    macroblock quantiser.  Both scale types, intra (I pictures) and non-intra (P pictures behind a flat I picture)"""
    rng = np.random.RandomState(7)
    pics, seen = [], set()
    for qst in (0, 1):
        for intra in (True, False):
            rows = []
            for k in range(1, 32):
                blocks = lambda: [(lv([(1, 3), (8, -2), (2, 1), (9, int(rng.randint(1, 4)))]), (100 + k) << 2 if intra else None)] * 6
                rows.append([dict(intra=intra, fwd=None if intra else (0, 0), cbp=63, blocks=blocks()),
                             dict(intra=intra, fwd=None if intra else (0, 0), cbp=63, quant=32 - k, blocks=blocks())])
                seen |= {(qst, "slice", k), (qst, "mb", 32 - k)}
            if not intra:
                pics.append(flat_i(128, 2, 31, qst=qst))
            pics.append(dict(type=1 if intra else 2, qst=qst, q=list(range(1, 32)), rows=rows))
    return case(build(32, 496, pics), ("scale_linear",), codes=len(seen))


@functools.lru_cache(maxsize=None)
def saturate_edges():
    """scale 2 (type 0, code 1) and weight 16: an intra level of +-1024 gives +-2048, a non-intra level of 1023 gives 2047, of -1024
    -2049, of 1024 2049 - at raster positions 1, 8 and 9, where the default intra matrix has 16 too"""
    found, seen = [], set()
    for intra, edges in ((True, ((1024, 2048), (-1024, -2048))), (False, ((1023, 2047), (-1024, -2049), (1024, 2049)))):
        ctx = ctx_of(intra)

        def gen(rng, intra=intra, edges=edges):
            l, value = edges[rng.randint(len(edges))]
            pairs = [(int(rng.randint(10, 64)), int(rng.randint(-40, 41))) for _ in range(int(rng.randint(0, 6)))] + [((1, 8, 9)[rng.randint(3)], l)]
            return dict(lv=lv(pairs), dc=int(rng.randint(300, 700)) if intra else None, q=1, value=value)
        got = search(11 + intra, gen, ctx, ("sat_symmetric", "sat_none"), each=3)
        seen |= {c["value"] for c in got}
        for l, value in edges:                                  # an edge no switch moves (2047 stays 2047) is in the stream all the same
            if value not in seen:
                got.append(dict(lv=lv([(1, l), (9, l)]), dc=512 if intra else None, q=1, value=value))
                seen.add(value)
        found.append((ctx, got))
    return case(pack(found), ("sat_symmetric", "sat_none"), values=tuple(sorted(seen)))


@functools.lru_cache(maxsize=None)
def mismatch():
    """non-intra blocks at scale 1 (type 1, code 1: F is the level) and scale 2 (F = 2 level +- 1, saturated), intra blocks at precision 3
    (intra_dc_mult 1: the DC can be odd).  holds: the classes of the issue's table that the chosen blocks fall into, from F before 7.4.4"""
    found, tags = [], set()

    def classify(c, ctx):
        F = samples(c, ctx, ("mm_none",))[1]
        even = int(F.sum()) % 2 == 0
        t = set()
        if even:
            t.add("even_f63_" + ("zero" if F[63] == 0 else "2047" if F[63] == 2047 else "-2048" if F[63] == -2048 else "odd" if F[63] & 1 else "even"))
        else:
            t.add("odd_sum")
        if (F < 0).any() and (F[F < 0] & 1).any():
            t.add("negative_odd")
        return t

    # (a), (b), (e): F is the level
    ctx = ctx_of(False, qst=1)

    def gen1(rng):
        pairs = [(int(rng.randint(0, 63)), int(rng.randint(-60, 61))) for _ in range(int(rng.randint(1, 8)))] + [(63, int((0, 0, 3, -5, 4, -6)[rng.randint(6)]))]
        c = dict(lv=lv(pairs), dc=None, q=1)
        return c if c["lv"].any() else None
    got = search(21, gen1, ctx, ("mm_none", "mm_always"), each=8)
    found.append((ctx, got))
    for c in got:
        tags |= classify(c, ctx)
    # (a) with F[63] = 2047 and -2048, (c): 2049 and -2049 change their parity in the saturation
    ctx = ctx_of(False, qst=0)

    def gen2(rng):
        pairs = [(int(rng.randint(0, 63)), int(rng.randint(-30, 31))) for _ in range(int(rng.randint(1, 8)))] + [(63, int((1023, -1024)[rng.randint(2)]))]
        if rng.randint(2):
            pairs.append((int(rng.randint(1, 10)), int((1024, -1024)[rng.randint(2)])))
        return dict(lv=lv(pairs), dc=None, q=1)
    got = search(22, gen2, ctx, ("mm_none", "mm_before_sat"), each=6)
    found.append((ctx, got))
    for c in got:
        tags |= classify(c, ctx)
    # (d): the DC alone decides
    ctx = ctx_of(True, qst=1, prec=3)

    def gen3(rng):
        pairs = [(int(rng.randint(1, 64)), 2 * int(rng.randint(-20, 21))) for _ in range(int(rng.randint(1, 8)))]
        return dict(lv=lv(pairs), dc=int(rng.randint(300, 1700)), q=2)          # scale 2, weights w: F = level w / 8 ...
    got = search(23, gen3, ctx, ("mm_no_dc",), each=6)
    found.append((ctx, got))
    for c in got:
        tags |= classify(c, ctx)
    return case(pack(found), ("mm_none", "mm_always", "mm_before_sat", "mm_no_dc"), classes=tuple(sorted(tags)))


@functools.lru_cache(maxsize=None)
def dc_precisions():
    """one I picture per precision: the DC predictors of the three components are driven to 0, to the legal top 2 ** (8 + precision) - 1,
    and to values in between, with AC coefficients beside them that bring samples back into 0 .. 255"""
    rng = np.random.RandomState(31)
    pics, seen = [], set()
    for prec in range(4):
        top = (1 << (8 + prec)) - 1
        values = [0, top, 0, top, top, 0, top, 1, top - 1, (100 << prec) + 1, (37 << prec) + (1 << prec) - 1, top // 2]
        rows = []
        for row in range(2):
            mbs = []
            for col in range(3):
                blocks = []
                for b in range(6):
                    dc = values[(7 * (3 * row + col) + 5 * b) % len(values)]
                    seen.add((prec, dc))
                    sign = 1 if dc < top // 2 else -1
                    blocks.append((lv([(1, sign * int(rng.randint(2, 9))), (8, sign * int(rng.randint(2, 9))), (int(rng.randint(2, 20)), int(rng.randint(-5, 6)))]), dc))
                mbs.append(dict(intra=True, blocks=blocks))
            rows.append(mbs)
        pics.append(dict(type=1, prec=prec, q=4, rows=rows))
    return case(build(48, 32, pics), ("dc_mult_wrong", "dc_offset_twice"), reached=tuple(sorted(seen)))


W_DISTINCT_I = tuple([8] + [2 + (37 * r) % 97 for r in range(1, 64)])
W_DISTINCT_N = tuple(120 + (29 * r) % 101 for r in range(64))


@functools.lru_cache(maxsize=None)
def weights_by_raster():
    """two custom matrices of distinct weights under the alternate scan"""
    assert len(set(W_DISTINCT_I[1:])) == 63 and len(set(W_DISTINCT_N)) == 64 and not set(W_DISTINCT_I) & set(W_DISTINCT_N)
    rng = np.random.RandomState(41)
    mb = lambda intra: dict(intra=intra, fwd=None if intra else (0, 0), cbp=63, blocks=[busy_block(rng, intra, most=10) for _ in range(6)])
    pics = [dict(type=1, alt=1, q=3, rows=[[mb(True) for _ in range(3)] for _ in range(2)]),
            dict(type=2, alt=1, q=2, rows=[[mb(False) for _ in range(3)] for _ in range(2)])]
    return case(build(48, 32, pics, seq=dict(intra_matrix=list(W_DISTINCT_I), non_intra_matrix=list(W_DISTINCT_N))), ("weight_by_scan", "matrices_swapped"))


@functools.lru_cache(maxsize=None)
def full_blocks():
    """16 x 48: 64 coefficients of +-2047 in the six sign patterns of dec_writer.SIGNS, scale codes 1, 16 and 31 down the rows: an I
    picture (DC at the legal top or 0 by the pattern's sign), and P pictures behind flat I pictures of 0, 128 and 255.  The two
    switches named for it cannot change a sample of ANY legal stream, and the case pins that: after the saturation of 7.4.3 the row pass
    stays within 2047 * (2048 + 2048 + 2841 + 2676 + 2408 + 1609 + 1108 + 565) / 256 < 2 ** 17, so 18 bits hold it; and a residual of
    -256 or -255 under a prediction of at most 255 ends at 0 either way"""
    def blocks(intra):
        out = []
        for name in W.SIGNS:
            sign = [W.SIGNS[name](r & 7, r >> 3) for r in range(64)]
            out.append((lv([(r, 2047 * sign[r]) for r in range(1 if intra else 0, 64)]), (1023 if sign[0] > 0 else 0) if intra else None))
        return out
    pics = [dict(type=1, q=[1, 16, 31], rows=[[dict(intra=True, blocks=blocks(True))] for _ in range(3)])]
    for base in (0, 128, 255):
        pics.append(flat_i(base, 1, 3))
        pics.append(dict(type=2, q=[1, 16, 31], rows=[[dict(fwd=(0, 0), cbp=63, blocks=blocks(False))] for _ in range(3)]))
    return case(build(16, 48, pics), (), equivalent=("row18", "clip255"))


@functools.lru_cache(maxsize=None)
def final_clip():
    """P pictures of DC-only residuals r (level 8 r at scale 1) over flat pictures of 1 and 254: prediction + residual of -2, -1, 0 and
    255, 256, 257; an I picture whose DCs and coefficients pass both ends too"""
    def p(rs):
        mbs = [dict(fwd=(0, 0), cbp=63, quant=1, blocks=[(lv([(0, 8 * r)]), None)] * 6) for r in rs]
        return dict(type=2, qst=1, q=1, rows=[mbs[:3], mbs[3:]])
    wide = dict(intra=True, blocks=[(lv([(1, 60), (8, -45)]), 40), (lv([(1, -60), (9, 30)]), 1000)] * 3)
    pics = [flat_i(1, qst=1), p((-3, -2, -1, 1, 2, 3)), flat_i(254, qst=1), p((3, 2, 1, -1, -2, -3)), dict(type=1, q=2, rows=[[wide] * 3] * 2)]
    return case(build(48, 32, pics), ("no_final_clip", "clip_high_only", "clip_low_only"))


# ---- prediction ----
@functools.lru_cache(maxsize=None)
def halfpel_rounding():
    """a busy I picture read at all four phases in luma, and with luma vectors of +-2 and +-3 at the half-sample phases of chroma"""
    rng = np.random.RandomState(51)
    p1 = dict(type=2, rows=[[moved((1, 0)), moved((0, 1)), moved((-1, 1))], [moved((2, -2)), moved((1, -1)), moved((-2, -3))]])
    p2 = dict(type=2, rows=[[moved((3, 3)), moved((2, 0)), moved((-3, 2), rng=rng, cbp=0b101011)], [moved((0, -2)), moved((-1, -1), rng=rng, cbp=63), moved((-3, -1))]])
    return case(build(48, 32, [busy_i(rng), p1, p2]), ("hp_trunc", "hp_plus1", "hp_two_stage"))


@functools.lru_cache(maxsize=None)
def chroma_vectors():
    """luma vectors -1, -3, +1, +3 in x and in y: -1 / 2 = 0 and -3 / 2 = -1 toward zero, -1 and -2 by a shift"""
    rng = np.random.RandomState(52)
    p1 = dict(type=2, rows=[[moved((1, 3)), moved((-1, 1)), moved((-3, 3))], [moved((3, -1)), moved((-1, -3)), moved((-3, -3))]])
    p2 = dict(type=2, rows=[[moved((3, 1)), moved((-3, 0)), moved((-1, 0))], [moved((0, -1)), moved((0, -3)), moved((-3, -1), rng=rng, cbp=0b000011)]])
    return case(build(48, 32, [busy_i(rng), p1, p2]), ("chroma_floor",))


def _busy_p(rng):
    return dict(type=2, q=3, rows=[[moved((1, 1), rng=rng, cbp=63), moved((-1, 0), rng=rng, cbp=63), moved((-2, 1), rng=rng, cbp=63)],
                                   [moved((0, -1), rng=rng, cbp=63), moved((1, -2), rng=rng, cbp=63), moved((-1, -1), rng=rng, cbp=63)]])


@functools.lru_cache(maxsize=None)
def b_mean():
    """I, P, B, B in coded order: both directions at every pair of phases, forward only and backward only beside them, with and
    without a residual"""
    rng = np.random.RandomState(53)
    b1 = dict(type=3, rows=[[moved((1, 0), (0, 1)), moved((1, 1), (0, 0)), moved((-1, 1), None)],
                            [moved(None, (1, -1)), moved((-1, -1), (1, -1)), moved((-2, -3), (-1, 0))]])
    b2 = dict(type=3, rows=[[moved((0, 0), (1, 1), rng=rng, cbp=63), moved((1, 0), (1, 1)), moved(None, (-3, 1), rng=rng, cbp=0b110000)],
                            [moved((1, -1), None, rng=rng, cbp=0b000111), moved((0, -1), (-1, 0)), moved((-1, -1), (-1, -1))]])
    return case(build(48, 32, [busy_i(rng), _busy_p(rng), b1, b2]), ("b_joint", "b_trunc", "b_swapped"), b=True)


@functools.lru_cache(maxsize=None)
def field_prediction():
    """48 x 32 of a sequence that is not progressive (two macroblock rows): an I picture with both dct_types, then P pictures with
    frame_pred_frame_dct 0: every pair of field selects, vertical half samples inside a field, negative odd field vectors, and coded
    macroblocks with dct_type 1"""
    rng = np.random.RandomState(54)
    F = lambda a, b, **kw: moved((a, b), motion="field", **kw)
    p1 = dict(type=2, field=True, rows=[[F((0, (1, 1)), (1, (0, 1))), F((1, (-1, 1)), (0, (-3, 3))), F((0, (-1, 0)), (0, (-3, 1)))],
                                        [F((1, (1, -1)), (1, (3, -3))), moved((0, 0), rng=rng, cbp=63, dct=1), F((0, (-1, -1)), (1, (-3, -3)), rng=rng, cbp=63, dct=1)]])
    p2 = dict(type=2, field=True, rows=[[F((1, (0, 3)), (0, (2, 1)), rng=rng, cbp=0b111100, dct=1), moved((1, 1), rng=rng, cbp=63, dct=0), F((1, (-2, 1)), (1, (-1, 2)))],
                                        [moved(None, rng=rng, cbp=0b110011, dct=1), F((0, (-1, -3)), (1, (1, -1))), F((1, (-3, -1)), (0, (0, -2)))]])
    selects = {(m["fwd"][0][0], m["fwd"][1][0]) for p in (p1, p2) for r in p["rows"] for m in r if m.get("motion") == "field"}
    return case(build(48, 32, [busy_i(rng, field=True), p1, p2]), ("field_vert_frame_row", "field_chroma_floor", "field_dct_frame_map"), i=True, selects=tuple(sorted(selects)))


CASES = dict(trunc_intra=trunc_intra, trunc_non_intra=trunc_non_intra, sign_term=sign_term, weights_1_255=weights_1_255, weights_1_255_qme=weights_1_255_qme,
             scale_codes=scale_codes, saturate_edges=saturate_edges, mismatch=mismatch, dc_precisions=dc_precisions, weights_by_raster=weights_by_raster,
             full_blocks=full_blocks, final_clip=final_clip, halfpel_rounding=halfpel_rounding, chroma_vectors=chroma_vectors, b_mean=b_mean,
             field_prediction=field_prediction)
NAMES = tuple(sorted(CASES))


def cases():
    return {name: CASES[name]() for name in NAMES}


@functools.lru_cache(maxsize=None)
def expected(name):
    """the plain reference's frames of a case, [n, frame bytes] of I420"""
    return R.flat(R.frames(CASES[name]()["log"]))


def settings(c):
    """the (b_pictures, interlaced, extended) settings of m2v_decode_device that accept a case's stream"""
    return [(b, i, x) for b in (False, True) for i in (False, True) for x in (False, True) if b >= c["b"] and i >= c["i"] and x >= c["x"]]


# ---- the accuracy stream (Annex A of 13818-2, IEEE 1180) ----
ACC = dict(w=640, h=416, n=1000, sets=((256, 255, 1), (256, 255, -1), (5, 5, 1), (5, 5, -1), (300, 300, 1), (300, 300, -1)))
ACC_LIMITS = dict(peak=1, position_mse=0.06, overall_mse=0.02, position_mean=0.015, overall_mean=0.0015)


@functools.lru_cache(maxsize=None)
def accuracy_coefficients():
    """the six sets -> [6, 1000, 64] coefficients in raster order: RandomState(1180 + L) draws 1000 blocks of integers in [-L, H]
    (sign-flipped for the second set of a pair), float64 forward DCT, rounded, clipped to -2048 .. 2047"""
    out = []
    for L, H, sign in ACC["sets"]:
        f = sign * np.random.RandomState(1180 + L).randint(-L, H + 1, size=(ACC["n"], 8, 8))
        out.append(np.clip(np.rint(R.fdct_real(f)), -2048, 2047).astype(np.int64))
    out = np.stack(out)
    assert out.min() >= -2047, "-2048 has no level (no set reaches it: eleven standard deviations)"
    return out


@functools.lru_cache(maxsize=None)
def accuracy():
    """640 x 416, pictures I, P, I, P: the I pictures flat at 1 and 254; macroblock k = 0 .. 999 of a P picture (rows 0 .. 24) holds block k
    of set b as its block b - non-intra, default matrix of 16, q_scale_type 1, scale code 1, so F is the level - with the zero vector,
    all-zero blocks left out of the pattern.  Row 25: macroblocks with one coded block each, the pattern going round, and "MC, not coded"
    ones: what is not coded must come out as the prediction (all-zero in, all-zero out).
    -> dict(stream, log, F [6, 1000, 64] after mismatch control, real [6, 1000, 8, 8] = idct_real(F), coded [6, 1000])"""
    C = accuracy_coefficients()
    coded = C.any(axis=2)
    rows = []
    for row in range(25):
        mbs = []
        for col in range(40):
            k = 40 * row + col
            cbp = sum(1 << (5 - b) for b in range(6) if coded[b, k])
            mbs.append(dict(fwd=(0, 0), cbp=cbp, blocks=[(C[b, k], None) for b in range(6) if coded[b, k]]))
        rows.append(mbs)
    rows.append([dict(fwd=(0, 0), cbp=1 << (col % 6), blocks=[(lv([(0, 16), (1, -9)]), None)]) if col % 7 else dict(fwd=(0, 0), cbp=0) for col in range(40)])
    p = dict(type=2, qst=1, q=1, rows=rows)
    s, log = build(ACC["w"], ACC["h"], [flat_i(1, 40, 26, qst=1), p, flat_i(254, 40, 26, qst=1), p])
    F = np.stack([R.mismatch(C[b]) for b in range(6)])
    F[~coded] = 0
    real = np.stack([R.idct_real(F[b]) for b in range(6)])
    return dict(stream=s, log=log, F=F, real=real, coded=coded)


def accuracy_residuals(frames):
    """the frames of the accuracy stream ([4, frame bytes] of I420) -> the residuals the decoder showed, [6, 1000, 8, 8]: from the first P
    picture (over 1) where the real transform is >= 0, else from the second (over 254)"""
    w, h = ACC["w"], ACC["h"]
    real = accuracy()["real"]
    got = []
    for pic, base in ((1, 1), (3, 254)):
        y = frames[pic][:w * h].reshape(h, w).astype(np.int64) - base
        u = frames[pic][w * h:w * h + w * h // 4].reshape(h // 2, w // 2).astype(np.int64) - base
        v = frames[pic][w * h + w * h // 4:].reshape(h // 2, w // 2).astype(np.int64) - base
        sets = []
        for b in range(4):
            part = y[:400].reshape(25, 2, 8, 40, 2, 8)[:, b >> 1, :, :, b & 1, :]          # [row, y, col, x]
            sets.append(part.transpose(0, 2, 1, 3).reshape(1000, 8, 8))
        for c in (u, v):
            sets.append(c[:200].reshape(25, 8, 40, 8).transpose(0, 2, 1, 3).reshape(1000, 8, 8))
        got.append(np.stack(sets))
    return np.where(real >= 0, got[0], got[1])


def accuracy_uncoded_ok(frames):
    """row 25 and every block left out of a pattern shows the prediction itself in both P pictures"""
    w, h = ACC["w"], ACC["h"]
    ok = True
    for pic, base in ((1, 1), (3, 254)):
        y = frames[pic][:w * h].reshape(h, w)
        c = frames[pic][w * h:].reshape(2, h // 2, w // 2)
        for col in range(40):
            coded = (1 << (col % 6)) if col % 7 else 0
            for b in range(6):
                blk = y[400 + 8 * (b >> 1):408 + 8 * (b >> 1), 16 * col + 8 * (b & 1):16 * col + 8 * (b & 1) + 8] if b < 4 else c[b - 4, 200:208, 8 * col:8 * col + 8]
                if not (coded >> (5 - b)) & 1:
                    ok = ok and bool((blk == base).all())
                else:
                    ok = ok and bool((blk != base).any())
    return ok


def accuracy_excluded():
    """[6, 1000, 8, 8]: samples left out - |idct_real| > 253, where the clip to 0 .. 255 would hide an error"""
    return np.abs(accuracy()["real"]) > 253


def accuracy_figures(residuals):
    """Annex A's figures per set over the samples kept: dict(peak, position_mse, overall_mse, position_mean, overall_mean), each [6]"""
    a = accuracy()
    keep = ~accuracy_excluded() & a["coded"][:, :, None, None]
    err = np.where(keep, residuals - a["real"], 0).astype(np.float64)
    n_pos = np.maximum(keep.sum(axis=1), 1)
    n_all = np.maximum(keep.sum(axis=(1, 2, 3)), 1)
    return dict(peak=np.abs(err).max(axis=(1, 2, 3)), position_mse=((err ** 2).sum(axis=1) / n_pos).max(axis=(1, 2)), overall_mse=(err ** 2).sum(axis=(1, 2, 3)) / n_all,
                position_mean=np.abs(err.sum(axis=1) / n_pos).max(axis=(1, 2)), overall_mean=np.abs(err.sum(axis=(1, 2, 3)) / n_all))


def accuracy_within(fig):
    return all((fig[k] <= ACC_LIMITS[k]).all() for k in ACC_LIMITS)


# ---- the host build of the dequantiser ----
_HARNESS = r"""
#include "dec_main_host.hpp"
extern "C" void arith_host_dequant(const int32_t *q, const int32_t *w, uint64_t n, int intra, int qscale, int32_t *out)
{
    for (uint64_t k = 0; k < n; ++k) out[k] = m2v::dec::main_dequant(q[k], w[k], intra != 0, qscale);
}
extern "C" void arith_host_dequant_dc(const int32_t *dc, uint64_t n, unsigned prec, int32_t *out)
{
    for (uint64_t k = 0; k < n; ++k) out[k] = m2v::dec::main_dequant_dc(dc[k], prec);
}
extern "C" int arith_host_scale(unsigned code, unsigned type) { return m2v::dec::main_scale(code, type); }
"""

_host = None


def host_lib():
    """dec::main_dequant, main_dequant_dc and main_scale of csrc/m2v_decode_kernels.hpp compiled with g++"""
    global _host
    if _host is None:
        import ctypes
        import os
        import subprocess
        import tempfile
        d = tempfile.mkdtemp(prefix="m2v_arith_host_")
        src, so = os.path.join(d, "arith_host.cpp"), os.path.join(d, "libarith_host.so")
        with open(src, "w") as f:
            f.write(_HARNESS)
        inc = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Werror", "-I", inc, "-I", os.path.join(D.ROOT, "tools"), "-o", so, src])
        L = ctypes.CDLL(so)
        L.arith_host_dequant.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        L.arith_host_dequant_dc.argtypes = [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint, ctypes.c_void_p]
        _host = L
    return _host


def host_dequant(q, w, intra, qscale):
    q, w = np.ascontiguousarray(q, np.int32), np.ascontiguousarray(w, np.int32)
    out = np.empty(q.shape, np.int32)
    host_lib().arith_host_dequant(q.ctypes.data, w.ctypes.data, q.size, int(intra), int(qscale), out.ctypes.data)
    return out.astype(np.int64)


def host_dequant_dc(dc, prec):
    dc = np.ascontiguousarray(dc, np.int32)
    out = np.empty(dc.shape, np.int32)
    host_lib().arith_host_dequant_dc(dc.ctypes.data, dc.size, prec, out.ctypes.data)
    return out.astype(np.int64)


class _Frames:
    def __init__(self, frames):
        self.frames = frames


@functools.lru_cache(maxsize=None)
def expected_in(name, layout="i420"):
    """expected(name) in one of the four 4:2:0 layouts, as m2v_decode_device writes them"""
    return D.frames_of(_Frames(R.frames(CASES[name]()["log"])), layout)
