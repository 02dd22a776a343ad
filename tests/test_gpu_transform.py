"""-m gpu: the arithmetic of k_mb between the decision and the codes - 4:4:4 -> 4:2:0, the forward transform on the matrix cores and on
the VALU path, the intra, DC and non-intra quantisers with their per-lane constants, the two inverse quantisers, the Chen-Wang inverse
transform, the final clip - on the clips of tests/transform_clips.py, against the oracle.

The other GPU tests reach this part of the kernel with whatever numbers their content produces.  Here every AC position of an intra tile
has a coefficient on either side of the boundaries of levels 1, 2, 3 and of the largest level whose boundary the search of
transform_clips.solve reaches from 8-bit samples, with both signs, in luma and in chroma, in I pictures and (level 1) in intra macroblocks of P pictures; the DC coefficient takes every residue mod 16 in
each of its roles; every position of a non-intra tile sits on either side of the boundaries of levels 1, 2, 3 in luma (matrix cores)
and in chroma (VALU); 2 x 2 chroma cells of every rounding class are subsampled; the sum in front of the final clip is -1, 0, 255 and
256, and the inverse transform leaves its own clip range both ways in intra and in non-intra tiles; mismatch control toggles and does
not.  The intra and non-intra boundaries run at every VECTOR_LEVEL: each of k_mb<VL, P>'s six lane tables is device data of its own.  tests/test_transform_clips.py (CPU) asserts from the oracle alone that the clips as committed
do all that, and that single-point faults of this arithmetic change what they produce.
Every clip is compared stage by stage on the -DM2V_DEBUG build (gpu_util.compare_stages names macroblock, tile and position of the first
level that differs, and compares the reconstruction of every referenced picture - the pictures with the targets are referenced) and byte
for byte on the shipped build, with the VALU transform (dct_mfma = 0) and in the conformant mode; one clip of every kind also through
the port interface, and one cut into strips of macroblock rows."""
import numpy as np
import pytest

import transform_clips as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", T.cases(), ids=T.case_id)
def test_clip_stage_by_stage_and_byte_for_byte(case):
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip, pf, VL, Q = T.make(*case)
    n, _, H, W = clip.shape
    ref = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, dump=True)
    # one chunk: the debug build keeps the dumps of its last chunk
    assert G.compare_stages(clip, W // 16, H // 16, pf, 7, 7, VL, Q, batch_frames=96, ref=ref) == []
    got = G.resident_encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    assert len(got) == len(ref[0]) and got == ref[0]


def encode_with(opts, clip, pf, VL, Q, port=False):
    import gpu_util as G
    n, _, H, W = clip.shape
    enc = G.M.Mpeg2Encoder(7, 7, VL, Q)
    try:
        for k, v in opts.items():
            enc.set_option(k, v)
        if port:
            return enc.encode(clip, W // 16, H // 16, pf)
        return G.resident_encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, enc=enc)
    finally:
        enc.close()


@pytest.mark.parametrize("case", T.cases(), ids=T.case_id)
def test_clip_with_the_valu_transform_and_in_conformant_mode(case):
    """option dct_mfma = 0 (every tile on the VALU path, the intra constants of every lane from the other table) against the oracle's
    stream; option conformant = 1 (truncating inverse quantiser, saturation, mismatch control, full-width row pass, -256 .. 255, tiles
    without levels not reconstructed) against the oracle's conformant stream"""
    from oracle import m2v_oracle_ctypes as orc
    clip, pf, VL, Q = T.make(*case)
    n, _, H, W = clip.shape
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    got = encode_with({"dct_mfma": 0}, clip, pf, VL, Q)
    assert len(got) == len(want) and got == want
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, conformant=True)
    got = encode_with({"conformant": 1}, clip, pf, VL, Q)
    assert len(got) == len(want) and got == want


PORT_CASES = [next(case for case in T.cases() if case[0] == kind and case[1] == Q) for kind, Q in
              (("intra", 1), ("intra_max", 2), ("inter", 3), ("intra_p", 4), ("subsample", T.SUBSAMPLE_Q), ("clipper", 2), ("intra_over", T.OVER_Q), ("extremes", 1))]


@pytest.mark.parametrize("case", PORT_CASES, ids=T.case_id)
def test_one_clip_of_every_kind_through_the_port_interface(case):
    from oracle import m2v_oracle_ctypes as orc
    clip, pf, VL, Q = T.make(*case)
    n, _, H, W = clip.shape
    for opts, conformant in (({}, False), ({"conformant": 1}, True)):
        want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, conformant=conformant)
        got = encode_with(opts, clip, pf, VL, Q, port=True)
        assert len(got) == len(want) and got == want, opts


STRIP_CASE = ("inter", 2, 2)


@pytest.mark.parametrize("world", [2, 3])
def test_the_inter_clip_as_strips_of_macroblock_rows(world):
    """m2v_strip_encode over the in-process communicator: the 12 macroblock rows of the clip cut before row 6 | rows 4 and 8; the
    neighbours' reconstruction rows of the picture with the targets feed the residuals of the picture behind it"""
    import torch
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    from test_gpu_strips import run_native_strips
    assert STRIP_CASE in T.cases()
    clip, pf, VL, Q = T.make(*STRIP_CASE)
    n, _, H, W = clip.shape
    d_clip = torch.from_numpy(np.ascontiguousarray(clip)).to("cuda:0")
    for conformant in (False, True):
        want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, conformant=conformant)
        got, stats = run_native_strips(G.M, d_clip, W, H, pf, VL, world, Q=Q, conformant=conformant)
        assert len(got) == len(want) and got == want, conformant
