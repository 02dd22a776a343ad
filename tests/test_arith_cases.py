"""The arithmetic of the main-syntax decoder on the CPU: the plain reference of tests/arith_ref.py - written from the standard's text,
fed from a log, never parsing - against the definition (decoder.decode(..., syntax="main")) and the host build of the device's
functions (tools/dec_x_host.hpp, g++) on every stream of tests/arith_cases.py; the proof that each case is sensitive to the rule it is
named after (the reference with that rule's switch thrown gives other frames); the dequantiser swept exhaustively; and the inverse
DCT's accuracy against the real transform by the criteria of 13818-2 Annex A (IEEE 1180).  tests/test_gpu_decode_arith.py runs the
same streams through every copy of the device's reconstruction kernel."""
import numpy as np
import pytest

import arith_cases as A
import arith_ref as R
import dec_cases as D
import ext_cases as X
import main_writer as MW

M = D.M
decoder = M.decoder


def test_tables_typed_apart_agree():
    """the scans, the scale table and the default matrix of the reference and the cases against decoder.py's and the writer's"""
    assert list(decoder.tables()["zz"]) == list(A.ZIGZAG) == R.zigzag()
    assert list(decoder._main_tables()["alt"]) == list(A.ALTERNATE)
    assert tuple(decoder.main_tables()["nonlinear"][1:]) == R.NONLINEAR == tuple(MW.NONLINEAR)
    assert tuple(decoder.iso_tables()["intra_w"]) == A.DEFAULT_INTRA == tuple(X.MW_default_intra())
    assert all(A.host_lib().arith_host_scale(c, t) == R.quantiser_scale(c, t) for c in range(1, 32) for t in (0, 1))


@pytest.mark.parametrize("name", A.NAMES)
def test_known_answers(name):
    """the plain reference's frames, built from the log without parsing, are the definition's on the stream - under the options the
    stream needs and under all three - and the host build's"""
    c = A.CASES[name]()
    want = A.expected(name)
    for b, i, x in ((c["b"], c["i"], c["x"]), (True, True, True)):
        d, at = X.spec(c["stream"], b, i, x)
        assert d is not None, (name, at)
        got = D.frames_of(d)
        assert got.shape == want.shape and np.array_equal(got, want), (name, np.nonzero(got != want))
    f, r = X.host_decode(c["stream"], c["b"], c["i"])
    assert r["status"] == D.OK and np.array_equal(f, want), (name, r)


@pytest.mark.parametrize("name", A.NAMES)
def test_every_mutant_is_caught(name):
    """each switch named for the case changes its frames; the switches listed as equivalent provably cannot (full_blocks says why)
    and do not"""
    c = A.CASES[name]()
    want = A.expected(name)
    assert c["mutants"] or c["equivalent"]
    for m in c["mutants"]:
        assert not np.array_equal(R.flat(R.frames(c["log"], m)), want), (name, m)
    for m in c["equivalent"]:
        assert np.array_equal(R.flat(R.frames(c["log"], m)), want), (name, m)


@pytest.mark.parametrize("name", A.NAMES)
def test_the_log_is_what_the_writer_wrote(name):
    """the writer's own log of the blocks it put into the stream - every (scan position, level) and every DC differential, in order -
    against the log the reference computes from"""
    log = A.CASES[name]()["log"]
    mine = [(mb["intra"], lv, diff) for pic in log["pictures"] for mb in pic["mbs"] for lv, diff in mb["blocks"]]
    wrote = log["writer"]["blocks"]
    diffs = iter(after - before for _, _, _, after, before, _ in log["writer"]["dc"])
    assert len(mine) == len(wrote) > 0
    for (intra, lv, diff), (w_intra, _, w_levels) in zip(mine, wrote):
        assert intra == w_intra and [(k, int(v)) for k, v in enumerate(lv) if v] == [(k, v) for k, v in w_levels]
        assert not intra or diff == next(diffs)
    assert next(diffs, None) is None


def test_every_switch_has_a_case():
    used = {m for name in A.NAMES for m in A.CASES[name]()["mutants"] + A.CASES[name]()["equivalent"]}
    assert used == set(R.MUTANTS)


def test_what_the_cases_hold():
    """from the builders' own counts, not from a decoder"""
    c = A.cases()
    assert c["weights_1_255"]["holds"]["largest"] == c["weights_1_255_qme"]["holds"]["largest"] == 4095 * 255 * 112
    assert c["scale_codes"]["holds"]["codes"] == 2 * 2 * 31                      # both types x (slice header, macroblock quantiser) x 31 codes
    assert c["saturate_edges"]["holds"]["values"] == (-2049, -2048, 2047, 2048, 2049)
    assert set(c["mismatch"]["holds"]["classes"]) >= {"even_f63_zero", "even_f63_odd", "even_f63_even", "even_f63_2047", "even_f63_-2048", "odd_sum", "negative_odd"}
    reached = set(c["dc_precisions"]["holds"]["reached"])
    assert all((p, 0) in reached and (p, (1 << (8 + p)) - 1) in reached for p in range(4))
    assert c["field_prediction"]["holds"]["selects"] == ((0, 0), (0, 1), (1, 0), (1, 1))
    assert all(len(x["stream"]) < 16384 for x in c.values())
    # trunc_*: negative products that are no multiple of 32 are all the AC content there is
    for name, intra in (("trunc_intra", True), ("trunc_non_intra", False)):
        log = c[name]["log"]
        n = 0
        for pic in log["pictures"]:
            for mb in pic["mbs"]:
                if mb["intra"] != intra:
                    continue
                for lv, _ in mb["blocks"]:
                    q = np.zeros(64, np.int64)
                    q[pic["scan"]] = lv
                    prod = (2 * q + (0 if intra else np.sign(q))) * np.array(pic["matrices"][0 if intra else 1]) * R.quantiser_scale(mb["qcode"], pic["qst"])
                    prod = prod[1:] if intra else prod
                    assert (prod <= 0).all() and (prod[prod < 0] % 32 != 0).all()
                    n += int((prod < 0).sum())
        assert n >= 36


def test_halfpel_sums_of_every_residue_are_read():
    """the reference picture of halfpel_rounding read at the phases its vectors name: a + b odd, and a + b + c + d of every residue mod 4, in
    luma and in chroma"""
    log = A.halfpel_rounding()["log"]
    ref = R.frames(dict(log, pictures=log["pictures"][:1]))[0]
    for p in (0, 1):
        a = ref[p].astype(np.int64)
        assert ((a[:, :-1] + a[:, 1:]) & 1).any() and ((a[:-1] + a[1:]) & 1).any()
        assert set(np.unique((a[:-1, :-1] + a[:-1, 1:] + a[1:, :-1] + a[1:, 1:]) & 3)) == {0, 1, 2, 3}
    phases = {p: set() for p in (0, 1)}
    for mb in log["pictures"][1]["mbs"] + log["pictures"][2]["mbs"]:
        x, y = mb["fwd"]
        phases[0].add((x & 1, y & 1))
        phases[1].add((int(x / 2) & 1, int(y / 2) & 1))
    assert phases[0] == phases[1] == {(0, 0), (1, 0), (0, 1), (1, 1)}


def test_where_32_bits_matter():
    """the Chen-Wang transform with integers of 32 bits (what ISO mode is) and with integers that never wrap give the same frames
    on every case but those whose blocks are far outside what a forward transform of samples produces: 64 coefficients of +-2047,
    weights of 255 on levels of +-2047, F[7][7] of 2047 beside coefficients of +-2048.  13818-2 gives a decoder no figure to meet
    there (Annex A measures blocks that come from samples of -256 .. 255, and 7.5 leaves the transform's arithmetic open); the
    project's definition is the 32-bit arithmetic, and the known answers hold it to that"""
    differ = {name for name in A.NAMES if not np.array_equal(R.flat(R.frames(A.CASES[name]()["log"], wrap32=False)), A.expected(name))}
    assert differ == {"full_blocks", "mismatch", "weights_1_255", "weights_1_255_qme"}


# ---- the dequantiser, exhaustively ----
SCALES = sorted({R.quantiser_scale(c, t) for c in range(1, 32) for t in (0, 1)})


def test_dequantiser_exhaustive():
    """every level -2047 .. 2047 x every weight 1 .. 255 x every distinct scale of both types x intra and non-intra: dec::main_dequant
    compiled with g++ against the plain reference's rule with 7.4.3's saturation - all 87.7 million of them; and decoder._main_dequant on
    every (weight, scale, kind) with 62 levels each, the levels going round so that every level meets it about 320 times (its
    coefficient loop is Python: the whole sweep would take minutes).  Its entries 1 .. 62 are compared: entry 0 of an intra block is
    the DC and entry 63 is where mismatch control acts"""
    assert len(SCALES) == 42 and SCALES[0] == 1 and SCALES[-1] == 112
    levels = np.arange(-2047, 2048, dtype=np.int64)
    q, w = np.meshgrid(levels, np.arange(1, 256, dtype=np.int64), indexing="ij")
    q, w = q.reshape(-1), w.reshape(-1)
    for intra in (True, False):
        for scale in SCALES:
            want = R.saturate(R.dequant_ac(q, w, intra, scale))
            assert np.array_equal(A.host_dequant(q, w, intra, scale), want), (intra, scale)
    for m in ("dq_floor", "sign_dropped", "prod24", "sat_symmetric"):       # the sweep sees what it is there for
        assert not np.array_equal(R.saturate(R.dequant_ac(q, w, False, 112, (m,)), (m,)), A.host_dequant(q, w, False, 112)), m
    at = 0
    for intra in (True, False):
        for scale in SCALES:
            for weight in range(1, 256):
                lv = levels[(at + np.arange(64)) % len(levels)].copy()
                lv[63] = 0
                at += 62
                got = decoder._main_dequant(lv, intra, scale, [weight] * 64, 1)
                want = R.saturate(R.dequant_ac(lv, weight, intra, scale))
                assert np.array_equal(got[1:63], want[1:63]), (intra, scale, weight)


def test_dequantiser_dc_exhaustive():
    """every legal DC of the four precisions: dec::main_dequant_dc and decoder._main_dequant, which keep the DC relative to the reset
    value, against intra_dc_mult x QF[0][0] of 7.4.1 less the 1024 that their prediction of 128 stands for"""
    for prec in range(4):
        dc = np.arange(0, 1 << (8 + prec), dtype=np.int64)
        want = R.dc_mult(prec) * dc - 1024
        assert want.min() == -1024 and want.max() == 1024 - R.dc_mult(prec)
        rel = dc - (1 << (7 + prec))
        assert np.array_equal(A.host_dequant_dc(rel, prec), want)
        for k in range(0, len(rel), 7 if prec else 1):
            QF = np.zeros(64, np.int64)
            QF[0] = rel[k]
            assert decoder._main_dequant(QF, True, 2, A.DEFAULT_INTRA, 8 >> prec)[0] == want[k]


# ---- the inverse DCT's accuracy, Annex A ----
ACC_EXCLUDED = (637, 635, 0, 0, 10007, 10007)


def test_idct_real_is_the_inverse():
    rng = np.random.RandomState(3)
    f = rng.randint(-256, 256, size=(50, 8, 8))
    assert np.array_equal(R.idct_real(R.fdct_real(f)), f)
    assert not R.idct_real(np.zeros((1, 64))).any() and not R.idct(np.zeros((1, 64), np.int64)).any()
    assert not decoder.idct(np.zeros(64, np.int64), False).any()


def test_annex_a():
    """The accuracy stream of arith_cases.accuracy() - six sets of 1000 blocks, (L, H) = (256, 255), (5, 5), (300, 300) and each
    sign-flipped, as non-intra blocks whose level is the coefficient - through decoder.py and through the host build, against
    idct_real with mismatch control on both sides.  Samples with |idct_real| > 253 are left out; their count per set is fixed by
    idct_real alone: 637, 635, 0, 0, 10007, 10007 of 64 000 (1.0 %, 0, 15.6 %).

    Measured (definition = host build = plain reference, byte for byte), per set in the order above:
        peak error                      1       1       1       1       1       1        (limit 1)
        worst position mean square      0.0242  0.0262  0.0120  0.0140  0.0239  0.0328   (limit 0.06)
        overall mean square             0.0153  0.0150  0.0068  0.0069  0.0161  0.0167   (limit 0.02)
        worst position mean, magnitude  0.0081  0.0111  0.0070  0.0060  0.0134  0.0119   (limit 0.015)
        overall mean, magnitude         0.00030 0.00058 0.00034 0.00003 0.00007 0.00011  (limit 0.0015)
    and a block that is not coded comes out as its prediction (all-zero in, all-zero out)"""
    a = A.accuracy()
    assert a["coded"].all() and tuple(int(v) for v in A.accuracy_excluded().sum(axis=(1, 2, 3))) == ACC_EXCLUDED
    want = R.flat(R.frames(a["log"]))
    assert (want[0] == 1).all() and (want[2] == 254).all()
    d, at = X.spec(a["stream"], False, False, False)
    assert d is not None, at
    host, r = X.host_decode(a["stream"], False, False)
    assert r["status"] == D.OK
    for name, frames in (("definition", D.frames_of(d)), ("host", host), ("reference", want)):
        fig = A.accuracy_figures(A.accuracy_residuals(frames))
        print(name, {k: np.round(v, 5).tolist() for k, v in fig.items()})
        assert A.accuracy_within(fig), (name, fig)
        assert A.accuracy_uncoded_ok(frames), name
        assert np.array_equal(frames, want), name
    # the yardstick itself: a decoder that is off by one somewhere in every block, or biased, fails
    biased = A.accuracy_residuals(want) + (np.arange(64).reshape(8, 8) == 27)
    assert not A.accuracy_within(A.accuracy_figures(biased))
