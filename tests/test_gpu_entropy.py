"""-m gpu: the entropy coder of k_mb - the symbol list of phase 8, the run/level look-up in both banks of d_ac_code2, the escapes, the
bit buffer - and the neighbour-dependent codes of mb_dependent / k_slice_scan / k_assemble, on the clips of tests/entropy_clips.py,
against the oracle.

The other GPU tests reach this part of the kernels with whatever symbols their content produces.  Here every run/level code of
table B-14 is coded in an intra macroblock and in both banks of a non-intra one, every run 0 .. 63 escapes with the first level that
has no code, levels sit on and past the clamps of the look-up, symbol lists end at 63, 64, 65, 127, 128 and 129 symbols and at the 387 /
391 that are the most a macroblock can hold, escapes and '1s' codes sit right behind the 64 symbols of a trip, every coded block
pattern is first in a slice and behind a neighbour, every DC differential is coded in each of its four roles and every vector delta
with its wrap, and slots hold exactly the bits of the class boundaries.  tests/test_entropy_clips.py (CPU) asserts from the oracle
alone that the clips as committed do all that.
Every clip is compared stage by stage on the -DM2V_DEBUG build (gpu_util.compare_stages names the first stage that differs: decision,
vectors, coded pattern, levels, reconstruction, bit lengths, bytes) and byte for byte on the shipped build; the clips of the codes,
the list indices and the slot sizes also through the port interface, with the VALU transform and in the conformant mode, and the
slot record k_mb leaves is compared with the census's."""
import numpy as np
import pytest

import entropy_clips as E

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", E.cases(), ids=E.case_id)
def test_clip_stage_by_stage_and_byte_for_byte(case):
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip, pf, VL, Q = E.make(*case)
    n, _, H, W = clip.shape
    ref = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, dump=True)
    # one chunk: the debug build keeps the dumps of its last chunk
    assert G.compare_stages(clip, W // 16, H // 16, pf, 7, 7, VL, Q, batch_frames=max(96, n), ref=ref) == []
    got = G.resident_encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    assert len(got) == len(ref[0]) and got == ref[0]


PATH_CASES = [case for case in E.cases() if case[0] in ("intra_codes", "inter_codes", "counts", "sizes")]


@pytest.mark.parametrize("case", PATH_CASES, ids=E.case_id)
def test_code_count_and_size_clips_port_interface_valu_transform_and_conformant_mode(case):
    """the same symbols whatever produced the levels: enc.encode (port interface) and option dct_mfma = 0 against the oracle's stream;
    option conformant = 1 against the oracle's conformant stream - there the reconstruction and with it the levels of the P pictures
    are other ones, which is wanted: more symbols, no census condition"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip, pf, VL, Q = E.make(*case)
    n, _, H, W = clip.shape
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    want_conformant = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, conformant=True)
    for opts, expect in (({}, want), ({"dct_mfma": 0}, want), ({"conformant": 1}, want_conformant)):
        enc = G.M.Mpeg2Encoder(7, 7, VL, Q)
        try:
            for k, v in opts.items():
                enc.set_option(k, v)
            got = G.resident_encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, enc=enc)
            assert len(got) == len(expect) and got == expect, opts
            got = enc.encode(clip, W // 16, H // 16, pf)
            assert len(got) == len(expect) and got == expect, (opts, "port interface")
        finally:
            enc.close()


SLOT_CASES = [case for case in E.cases() if case[0] in ("counts", "sizes")]


@pytest.mark.parametrize("case", SLOT_CASES, ids=E.case_id)
def test_slot_record_is_the_census_slot_bits(case):
    """the three segment lengths k_mb leaves in its aux record (m2v_debug_read 5) against the census: their sum is the census's slot
    bits on every macroblock - 255 .. 258, 511 .. 514 and 1023 .. 1026 bits among them, and the lists of 387 and 391 symbols - and
    each segment is the census's (A | B = AC of U | C = AC of V: the offsets pass 2 takes at idxB and idxC)"""
    import gpu_util as G
    clip, pf, VL, Q = E.make(*case)
    n, _, H, W = clip.shape
    mbs = (W // 16) * (H // 16)
    c = E.census_of(*case)
    enc = G.M.Mpeg2Encoder(7, 7, VL, Q)
    try:
        got = G.resident_encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, enc=enc)
        aux = enc.debug_read(5, n * mbs * 16, np.uint32).reshape(n, mbs, 4).astype(np.int64)
    finally:
        enc.close()
    assert got == c["bytes"]
    seg = np.stack([aux[:, :, 0] & 0xFFFF, aux[:, :, 0] >> 16, aux[:, :, 1] & 0xFFFF], -1)
    assert np.array_equal(seg.sum(-1), c["slot_bits"]), "first difference at (frame, macroblock) %s" % (np.argwhere(seg.sum(-1) != c["slot_bits"])[:1],)
    assert np.array_equal(seg, c["seg"]), "first difference at (frame, macroblock, segment) %s" % (np.argwhere(seg != c["seg"])[:1],)
