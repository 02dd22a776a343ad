"""An independent reference of the deinterlacer's definition (include/m2v_mi355x.h: m2v_deinterlace_device), written sample by sample in
plain Python integers: every output sample is computed on its own from the call's bytes - no arrays, no sequence of fields, nothing shared
with deinterlace_frames or with csrc/m2v_deint_kernels.hpp.  deinterlace(..., wrong=NAME) computes one of the classic wrong forms
instead; tests/test_deint_cases.py shows for each that the cases tell it from the definition."""

WRONG = (
    "parity swapped",                   # 1  the kept rows are those of the other field
    "order ignored",                    # 2  every call read as top field first
    "sp truncates",                     # 3  (c + e) >> 1
    "edge row from the other field",    # 4  a row missing at the plane's edge replaced by the row itself instead of the kept row beside it
    "edge row left as it is",           # 4  ... or the output row at the edge simply woven
    "absent field: the adjacent one",   # 5  a field outside the call replaced by the nearest field, whatever its parity
    "t0 not halved",                    # 6
    "t1 t2 not halved",                 # 7
    "one-sided clamp",                  # 8  max(sp, d - m) alone
    "chroma rows with luma parity",     # 9  chroma row r given the parity of the luma rows it covers, (2 r) & 1
    "nv12 as a plane of cw bytes",      # 10 the interleaved chroma plane cut into rows of cw bytes
    "field rate in parity order",       # 11 the two outputs of a frame top field first, whatever the order
    "blend without the + 2",            # 12
)


def _planes(w, h, layout, wrong):
    """[(offset, bytes of a row, rows, chroma?)]"""
    cw, ch = (w + 1) // 2, (h + 1) // 2
    if layout in ("i420", "yv12") or wrong == "nv12 as a plane of cw bytes":
        return [(0, w, h, False), (w * h, cw, ch, True), (w * h + cw * ch, cw, ch, True)]
    return [(0, w, h, False), (w * h, 2 * cw, ch, True)]


def deinterlace(frames, w, h, layout="i420", mode="adaptive", rate="frame", order="tff", wrong=None):
    """frames: the call's bytes (n whole frames) -> the output's bytes"""
    assert wrong is None or wrong in WRONG
    assert layout in ("i420", "yv12", "nv12", "nv21") and mode in ("line", "adaptive", "blend") and rate in ("frame", "field") and order in ("tff", "bff")
    assert not (mode == "blend" and rate == "field")
    src = bytes(frames)
    fb = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
    n = len(src) // fb
    assert n * fb == len(src)
    nfields = 2 * n
    first = {"tff": 0, "bff": 1}[order]
    out = bytearray((2 * n if rate == "field" else n) * fb)

    def inside(k):
        """the field that stands for field k"""
        if wrong == "absent field: the adjacent one":
            return min(max(k, 0), nfields - 1)
        while k < 0:
            k += 2
        while k >= nfields:
            k -= 2
        return k

    for j in range(len(out) // fb):
        if rate == "frame":
            k = 2 * j
        elif wrong == "field rate in parity order":
            k = 2 * (j >> 1) + ((j & 1) ^ first)
        else:
            k = j
        p = (k & 1) if wrong == "order ignored" else first ^ (k & 1)
        if wrong == "parity swapped":
            p ^= 1
        for off, rb, H, is_chroma in _planes(w, h, layout, wrong):
            def S(frame, y, x):
                return src[frame * fb + off + y * rb + x]
            for y in range(H):
                for x in range(rb):
                    f = k >> 1
                    if H < 2:
                        v = S(f, y, x)
                    elif mode == "blend":
                        v = (S(f, max(y - 1, 0), x) + 2 * S(f, y, x) + S(f, min(y + 1, H - 1), x) + (0 if wrong == "blend without the + 2" else 2)) >> 2
                    else:
                        parity = (2 * y) & 1 if is_chroma and wrong == "chroma rows with luma parity" else y & 1
                        at_edge = y - 1 < 0 or y + 1 >= H
                        if parity == p or (at_edge and wrong == "edge row left as it is"):
                            v = S(f, y, x)
                        else:
                            if wrong == "edge row from the other field":
                                yc, ye = max(y - 1, 0), min(y + 1, H - 1)
                            else:
                                yc = y - 1 if y - 1 >= 0 else y + 1
                                ye = y + 1 if y + 1 < H else y - 1
                            c, e = S(f, yc, x), S(f, ye, x)
                            v = (c + e + (0 if wrong == "sp truncates" else 1)) >> 1
                            if mode == "adaptive":
                                def T(kk, row):
                                    """the sample of row `row` in the frame that holds the field standing for field kk (the wrong form
                                    reads the adjacent field's own line at that height, one row off)"""
                                    g = inside(kk)
                                    if wrong == "absent field: the adjacent one" and ((g ^ kk) & 1):
                                        row = min(2 * (row >> 1) + (first ^ (g & 1)), H - 1)
                                    return S(g >> 1, row, x)
                                b, a = T(k - 1, y), T(k + 1, y)
                                d = (b + a) >> 1
                                t0 = abs(b - a) if wrong == "t0 not halved" else abs(b - a) >> 1
                                m = t0
                                for kk in (k - 2, k + 2):
                                    t = abs(T(kk, yc) - c) + abs(T(kk, ye) - e)
                                    m = max(m, t if wrong == "t1 t2 not halved" else t >> 1)
                                v = max(v, d - m)
                                if wrong != "one-sided clamp":
                                    v = min(v, d + m)
                    out[j * fb + off + y * rb + x] = v
    return bytes(out)
