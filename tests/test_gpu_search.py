"""-m gpu: the decision side of k_mb - full-pel search, half-pel refinement, the ten-way decision, luma and chroma prediction - on the
clips of tests/search_clips.py, against the oracle.

The other GPU tests reach this part of the kernel with whatever vectors their content produces.  Here every legal vector is chosen
by some macroblock, in the interior and on every edge and corner (all_vectors); every full-pel candidate is a member of a tie that
only the scan order decides, and every pair of half-pel positions ties at the minimum (ties); the intra cost ties with the best
half-pel SAD and lies one unit to either side of it (intra_tie); border macroblocks have their match on masked candidates (outward).
tests/test_search_clips.py (CPU) asserts from the oracle alone that the clips as committed do all that.
Every clip is compared stage by stage on the -DM2V_DEBUG build (gpu_util.compare_stages names the first stage that differs: decision,
vectors, coded pattern, levels, reconstruction, bit lengths, bytes) and byte for byte on the shipped build; the interior and ties
clips also through the port interface, with the VALU transform, in the conformant mode and cut into strips of macroblock rows."""
import numpy as np
import pytest

import search_clips as S

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", S.cases(), ids=S.case_id)
def test_clip_stage_by_stage_and_byte_for_byte(case):
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    kind, VL, Q, args = case
    clip, pf = S.make(*case)
    n, _, H, W = clip.shape
    ref = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, dump=True)
    # one chunk: the debug build keeps the dumps of its last chunk, and the edge and corner clips are hundreds of small frames
    assert G.compare_stages(clip, W // 16, H // 16, pf, 7, 7, VL, Q, batch_frames=max(96, n), ref=ref) == []
    got = G.resident_encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    assert len(got) == len(ref[0]) and got == ref[0]


PATH_CASES = [(kind, VL, S.Q_LEVELS[seed % 2], seed) for VL in S.VECTOR_LEVELS for kind in ("interior", "ties") for seed in (0, 1)]


@pytest.mark.parametrize("kind,VL,Q,seed", PATH_CASES)
def test_interior_and_ties_clips_port_interface_valu_transform_and_conformant_mode(kind, VL, Q, seed):
    """the same decisions whatever comes after them: enc.encode (port interface), option dct_mfma = 0, and option conformant = 1 -
    where the four-sample mean rounds with + 2 and the chroma vector truncates toward zero, so the half-pel SADs, the ties and the
    chroma phases are other ones - against the oracle's conformant mode"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    assert (kind, VL, Q, (seed,)) in S.cases()
    clip, pf = S.make(kind, VL, Q, (seed,))
    n, _, H, W = clip.shape
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    want_conformant = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, conformant=True)
    # (the streams differ except for the interior clips at Q_LEVEL 4, whose residuals quantise to nothing in either mode)
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


@pytest.mark.parametrize("world", [2, 3])
@pytest.mark.parametrize("kind,VL,Q,seed", PATH_CASES)
def test_interior_and_ties_clips_as_strips_of_macroblock_rows(kind, VL, Q, seed, world):
    """m2v_strip_encode over the in-process communicator (the fused edge-row kernel; with conformant = 1 the general form of the step)
    and over the peer transport (k_mb<.., EDGE, PEER>).  The interior clips are 11 / 19 / 27 macroblock rows: with 2 and 3 strips the
    boundaries fall before rows 6 | 4, 8 (VECTOR_LEVEL 1), 10 | 7, 13 (2), 14 | 9, 18 (3), and over the two seeds the rows next to
    them hold macroblocks with every vertical component that reads the neighbouring strip: mvy = 1 .. 4 VL in a strip's last row,
    -4 VL .. -1 in a strip's first row (asserted on the CPU: tests/test_search_clips.py
    ::test_interior_clips_carry_every_vertical_component_across_the_strip_boundaries)."""
    import torch
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    from test_gpu_strips import run_native_strips
    from test_gpu_strip_peer import run_peer_threads
    M = G.M
    clip, pf = S.make(kind, VL, Q, (seed,))
    n, _, H, W = clip.shape
    want = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q)
    d_clip = torch.from_numpy(np.ascontiguousarray(clip)).to("cuda:0")
    got, stats = run_native_strips(M, d_clip, W, H, pf, VL, world, Q=Q)
    assert len(got) == len(want) and got == want
    if seed == 0:
        want_conformant = orc.encode(clip, W // 16, H // 16, pf, 7, 7, VL, Q, conformant=True)
        got, stats = run_native_strips(M, d_clip, W, H, pf, VL, world, Q=Q, conformant=True)
        assert len(got) == len(want_conformant) and got == want_conformant
    got, stats, forms = run_peer_threads(M, d_clip, W, H, pf, VL, world, Q=Q)
    assert len(got) == 1 and len(got[0]) == len(want) and got[0] == want, (stats, forms)
    assert len({(s["peer_sequences"], s["giveups"], s["fell_back"]) for s in stats}) == 1, "the ranks disagree about what happened: %r" % (stats,)
