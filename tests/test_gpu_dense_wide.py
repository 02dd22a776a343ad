"""-m gpu: dense content on wide frames, and VECTOR_LEVEL 1 / 2 at full size, byte for byte against the oracle.

The other GPU tests run wide frames with tame content (synth.clip: nearly every macroblock in the two smallest slot classes, every
slice one pass of k_assemble) or dense content on narrow frames (at most 16 macroblocks per slice, all in one class).  Here the clips
of tests/dense_clips.py run at 33 .. 128 macroblocks per slice; tests/test_dense_clips.py (CPU) shows from the oracle alone that they
reach what they are for:
  * k_mb's four slot classes mixed inside every slice, sizes on both sides of the 256 / 512 / 1024-bit boundaries (mix, ramp);
  * k_assemble's staging filling inside the slice, unstaged compact slots next to overflow slots (mix at >= 120 macroblocks), compact
    slots alone over-filling it (uniform noise at Q_LEVEL 4 at >= 64), and 33 compact slots that fill it at the last macroblock in
    some slices and not in others ("brim"; uniform noise at Q_LEVEL 4 at 33 stays just under it by the kernel's own count);
  * slices of 3 - 5 passes (mix) and of 17 passes, 68 KB, every macroblock in the overflow class, bit offsets past 2^19 across the
    two-wavefront scans (binary noise at Q_LEVEL 1);
  * the host side: a sparse chunk followed by a multi-megabyte one on the same handle (the read-back buffer grows), the FIFO residue
    with dense words, strips whose sizes differ by large factors through the sizes all-gather and the gather to rank 0;
  * the re-dealt full-pel search of VECTOR_LEVEL 1 and 2 at 1920x1152 and at config c5's strip geometry through the edge-row kernel.
Wide-and-short cases are compared stage by stage on the -DM2V_DEBUG build (gpu_util.compare_stages names the first stage that differs)
and byte for byte on the shipped build: two compilations of the same sources.  The oracle runs once per (clip, parameters).

Wall time on one MI355X (measured once, 83 cases here, 312 in the suite): this file 22.5 s on its own, most of it the oracle; the whole
-m gpu suite 239.7 s with it, 217 s without (190.9 s is the figure recorded when the suite had 176 cases)."""
import json
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import dense_clips as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

@pytest.mark.parametrize("mbw,ys16,content,VL,Q,pf", D.wide_short_cases())
def test_wide_and_short_dense_slices(mbw, ys16, content, VL, Q, pf):
    """k_mb's slot classes (m2v_kernels.hpp: the store by word count), k_slice_scan / k_assemble's two-wavefront scans, staging and
    passes, on both builds"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip = D.wide_short_clip(mbw, ys16, content, Q)
    ref = orc.encode(clip, mbw, ys16, pf, 7, 7, VL, Q, dump=True)
    assert G.compare_stages(clip, mbw, ys16, pf, 7, 7, VL, Q, ref=ref) == []
    got = G.resident_encode(clip, mbw, ys16, pf, 7, 7, VL, Q)
    assert len(got) == len(ref[0]) and got == ref[0]


# ---- chunking and launch shape on dense data ----
def test_mix_clip_2048x128_chunking_streams_and_launch_shape():
    """the mix clip (all four classes and an over-full staging in every slice), 2 GOPs + 1 frame: the same bytes whatever the chunk
    length (a chunk of one frame, of a GOP, of everything), the number of streams, the block order of k_mb (cu_pack) and the luma
    transform path"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    W, H, pf, n = 2048, 128, 3, 9
    clip = D.mix(W, H, n, 12)
    want = orc.encode(clip, 128, 8, pf, 7, 7, 3, 2)
    variants = [{"batch_frames": 1}, {"batch_frames": 4}, {"batch_frames": 96}, {"batch_frames": 96, "split_streams": 1},
                {"batch_frames": 4, "split_streams": 3}, {"batch_frames": 96, "cu_pack": 0}, {"batch_frames": 4, "cu_pack": 3, "split_streams": 3},
                {"batch_frames": 4, "dct_mfma": 0}]
    for opts in variants:
        enc = G.M.Mpeg2Encoder(7, 7, 3, 2)
        try:
            for k, v in opts.items():
                enc.set_option(k, v)
            got = G.resident_encode(clip, 128, 8, pf, 7, 7, 3, 2, enc=enc)
            assert len(got) == len(want) and got == want, opts
            assert enc.encode(clip, 128, 8, pf) == want, (opts, "port interface")
        finally:
            enc.close()


# ---- full size ----
@pytest.fixture(scope="module")
def full_size_binary_noise():
    """1920x1152, first GOP (1 I + 8 P) of binary noise, VECTOR_LEVEL 3, Q_LEVEL 1: the clip and the oracle's stream, once for the
    two tests that need them (about 10 s of CPU here)"""
    from oracle import m2v_oracle_ctypes as orc
    clip = D.binary_noise(1920, 1152, 9, 5)
    return clip, orc.encode(clip, 120, 72, 8, 7, 7, 3, 1)


def test_1920x1152_binary_noise_first_gop_vs_oracle(full_size_binary_noise):
    """72 slices of 120 macroblocks, about 64 KB each, every macroblock in the overflow class: about 4.6 MB per frame"""
    import gpu_util as G
    clip, want = full_size_binary_noise
    assert len(want) > 9 * 4000000
    got = G.resident_encode(clip, 120, 72, 8, 7, 7, 3, 1)
    assert len(got) % 32 == 0
    assert len(got) == len(want) and got == want
    assert G.resident_encode(clip, 120, 72, 8, 7, 7, 3, 1, batch_frames=5) == want


def test_2048x2048_uniform_noise_q1_the_largest_output_per_frame():
    """XL = YL = 7 maximum frame, 1 I + 2 P of uniform noise at Q_LEVEL 1: 128 slices of 128 macroblocks, about 55 KB each"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip = D.noise(2048, 2048, 3, 6)
    want = orc.encode(clip, 128, 128, 2, 7, 7, 3, 1)
    got = G.resident_encode(clip, 128, 128, 2, 7, 7, 3, 1)
    assert len(got) == len(want) and got == want


def test_1920x1152_vector_levels_1_and_2_first_gop_vs_oracle():
    """the re-dealt full-pel search of k_mb<1, ...> / k_mb<2, ...> at full size: synth.clip content, first GOP byte-identical and
    chunking-invariant"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    W, H, pf = 1920, 1152, 8
    clip = G.M.synth.clip(W, H, pf + 1, clip_index=43)
    for VL, Q in ((1, 2), (2, 2), (1, 4), (2, 1)):
        want = orc.encode(clip, 120, 72, pf, 7, 7, VL, Q)
        got = G.resident_encode(clip, 120, 72, pf, 7, 7, VL, Q)
        assert len(got) == len(want) and got == want, (VL, Q)
        assert G.resident_encode(clip, 120, 72, pf, 7, 7, VL, Q, batch_frames=5) == want, (VL, Q, "batch_frames 5")


def test_1920x1152_vector_level_1_q1_on_the_mix_clip():
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip = D.mix(1920, 1152, 9, 13)
    want = orc.encode(clip, 120, 72, 8, 7, 7, 1, 1)
    got = G.resident_encode(clip, 120, 72, 8, 7, 7, 1, 1)
    assert len(got) == len(want) and got == want


# ---- port path ----
def pull_through_a_small_window(enc, clip, xs16, ys16, pf, per_push, cap, total):
    """m2v_push_frames_pull with a destination of `cap` bytes per call (smaller than a chunk: words queue up in the FIFO behind it),
    then m2v_pull until the last word"""
    out = np.zeros(total + 4096, np.uint8)
    pos, last = 0, False
    for k in range(0, clip.shape[0], per_push):
        m, last = enc.push_frames_pull(xs16, ys16, pf, clip[k:k + per_push], out[:min(out.size, pos + cap)], pos)
        pos += m
        assert not last
    enc.sequence_stop()
    for _ in range(total // cap + 64):                   # (bounded: a pull that stopped delivering must fail, not spin)
        if last:
            break
        m, last = enc.pull_into(out[:min(out.size, pos + cap)], pos)
        pos += m
    assert last
    return out[:pos].tobytes()


def test_one_handle_sparse_then_dense_then_sparse_through_the_ports(full_size_binary_noise):
    """m2v_port.hip: d_out sized per chunk, the pinned read-back buffer re-allocated when a chunk outgrows the previous one.  A flat
    1920x1152 sequence (a few KB per chunk), the binary-noise GOP (about 14 MB per chunk of three frames), the flat one again - on
    one handle, through enc.encode and through m2v_push_frames_pull with a 1 MB destination."""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    dense, want_dense = full_size_binary_noise
    sparse = D.flat(1920, 1152, 3)
    want_sparse = orc.encode(sparse, 120, 72, 8, 7, 7, 3, 1)
    assert len(want_sparse) < 100000 < 10000000 < len(want_dense)
    enc = G.M.Mpeg2Encoder(7, 7, 3, 1)
    try:
        enc.set_option("batch_frames", 3)
        for clip, want in ((sparse, want_sparse), (dense, want_dense), (sparse, want_sparse)):
            got = enc.encode(clip, 120, 72, 8)
            assert len(got) == len(want) and got == want
        for clip, want in ((sparse, want_sparse), (dense, want_dense), (sparse, want_sparse)):
            got = pull_through_a_small_window(enc, clip, 120, 72, 8, 3, 1 << 20, len(want))
            assert len(got) == len(want) and got == want
            assert not enc.busy
    finally:
        enc.close()


def test_nv12_noise_2048x64_resident():
    """one 4:2:0 case: NV12 noise through m2v_encode_resident420 against the oracle on the frames it stands for"""
    import torch
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    W, H, n, pf = 2048, 64, 4, 3
    x = np.random.default_rng(31).integers(0, 256, (n, W * H * 3 // 2), dtype=np.uint8)
    want = orc.encode(G.M.to444(x, W, H, "nv12"), 128, 4, pf, 7, 7, 3, 1)
    enc = G.M.Mpeg2Encoder(7, 7, 3, 1)
    try:
        d_in = torch.from_numpy(x).to("cuda:0")
        d_out = torch.empty(n * W * H * 3 + (1 << 16), dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        nb = enc.encode_resident420(d_in.data_ptr(), n, d_out.data_ptr(), d_out.numel(), 128, 4, pf, "nv12")
        got = d_out[:nb].cpu().numpy().tobytes()
        assert len(got) == len(want) and got == want
    finally:
        enc.close()


# ---- strips ----
PEER_CHILD = r'''
import json, sys
import numpy as np
root, clip_path, want_path, params = sys.argv[1:5]
sys.path.insert(0, root); sys.path.insert(0, root + "/tests")
import torch
import m2v_load
from test_gpu_strip_peer import run_peer_threads
M = m2v_load.load()
W, H, pf, VL, world, Q, calls = json.loads(params)
want = open(want_path, "rb").read()
d_clip = torch.from_numpy(np.load(clip_path)).to("cuda:0")
got, stats, forms = run_peer_threads(M, d_clip, W, H, pf, VL, world, calls=calls, Q=Q)
print("RESULT " + json.dumps({"identical": [g == want for g in got], "stats": stats, "forms": forms}))
'''


def peer_threads_with_a_queue_per_rank(tmp_path, clip, want, W, H, pf, VL, world, Q, calls):
    """run_peer_threads in a process of its own that asks the HIP runtime for sixteen hardware queues (GPU_MAX_HW_QUEUES is read when
    the runtime starts): with the default four, the ranks' launches wait behind each other's waiting blocks, a wait runs out of
    budget and the sequence is encoded again through the base communicator - the oracle's bytes either way, but not through
    k_mb<.., EDGE, PEER>.  So the form is asserted, not only the bytes: every call of every rank ran in the peer form, nobody gave up."""
    (tmp_path / "child.py").write_text(PEER_CHILD)
    np.save(tmp_path / "clip.npy", np.ascontiguousarray(clip))
    (tmp_path / "want.bin").write_bytes(want)
    env = dict(os.environ, GPU_MAX_HW_QUEUES="16")
    r = subprocess.run([sys.executable, str(tmp_path / "child.py"), ROOT, str(tmp_path / "clip.npy"), str(tmp_path / "want.bin"),
                        json.dumps([W, H, pf, VL, world, Q, calls])], env=env, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    print("peer transport, %d ranks, sixteen hardware queues:" % world, res["stats"][0], res["forms"])
    assert res["identical"] == [True] * calls, res
    assert all(s == {"peer_sequences": calls, "giveups": 0, "fell_back": False} for s in res["stats"]), res["stats"]
    assert set(res["forms"]) == {"peer"}, res["forms"]


def test_config_c5_geometry_vector_levels_1_and_2_through_the_strip_kernels(tmp_path):
    """2048x2048, 8 ranks x 16 macroblock rows as threads, one GOP of 1 I + 3 P.  VECTOR_LEVEL 1 through the peer transport, in the
    peer form for real (k_mb<1, .., EDGE, PEER> stores the neighbours' rows itself: asserted, see the helper); VECTOR_LEVEL 2 through
    the local communicator (the fused edge-row kernel, m2v_strips.hip)."""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    from test_gpu_strips import run_native_strips
    M = G.M
    W = H = 2048
    pf, n = 3, 4
    d_clip = M.synth.clip_torch(W, H, n, clip_index=59, device="cuda:0", scene_len=3)      # a scene cut inside the GOP
    clip = d_clip.cpu().numpy()
    want = orc.encode(clip, 128, 128, pf, 7, 7, 1, 2)
    peer_threads_with_a_queue_per_rank(tmp_path, clip, want, W, H, pf, 1, 8, 2, 2)
    want = orc.encode(clip, 128, 128, pf, 7, 7, 2, 2)
    got, stats = run_native_strips(M, d_clip, W, H, pf, 2, 8)
    assert len(got) == len(want) and got == want
    assert all(s["steps"] == pf + 1 for s in stats)


def test_strips_of_very_unequal_sizes_native_loop_and_peer_transport(tmp_path):
    """m2v_strips.hip: the sizes all-gather, the gather to rank 0 and its assembly.  2048x256, 4 ranks x 4 rows, Q_LEVEL 1, 1 I + 3 P:
    rank 0's rows flat, rank 1's the mix clip, rank 2's binary noise, rank 3's the mix clip - strips that differ by large factors in
    bytes, and the halo rows of a noise strip next to a flat one.  The native loop over the local communicator, then the peer
    transport, twice on one communicator, in the peer form (asserted)."""
    import torch
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    from test_gpu_strips import run_native_strips
    M = G.M
    W, H, pf, n = 2048, 256, 3, 4
    assert M.parallel.partition_rows(H // 16, 4) == [(0, 4), (4, 8), (8, 12), (12, 16)]
    clip = np.concatenate([D.flat(W, 64, n), D.mix(W, 64, n, 14), D.binary_noise(W, 64, n, 15), D.mix(W, 64, n, 16)], axis=2)
    want, d = orc.encode(clip, 128, 16, pf, 7, 7, 3, 1, dump=True)
    per_rank = d["mb_bits"].astype(np.int64).reshape(n, 4, -1).sum((0, 2)) // 8
    print("strip bytes per rank:", per_rank)
    assert per_rank[2] > 50 * per_rank[0] and per_rank[2] > 2 * per_rank[1]
    d_clip = torch.from_numpy(np.ascontiguousarray(clip)).to("cuda:0")
    got, stats = run_native_strips(M, d_clip, W, H, pf, 3, 4, Q=1)
    assert len(got) == len(want) and got == want
    peer_threads_with_a_queue_per_rank(tmp_path, clip, want, W, H, pf, 3, 4, 1, 2)


# ---- the CPU side's measure against the kernel's ----
@pytest.mark.parametrize("content,mbw,Q,pf", [("mix", 128, 2, 3), ("brim", 33, 2, 3), ("noise", 65, 4, 0), ("ramp", 127, 1, 3)])
def test_slot_bits_is_what_k_mb_stored(content, mbw, Q, pf):
    """dense_clips.slot_bits (the oracle's mb_bits less the neighbour-dependent codes, numpy) against the three segment lengths k_mb
    left in its aux record (m2v_debug_read 5): equal for every macroblock, intra and inter, so that "by the kernel's own count" in
    tests/test_dense_clips.py is the kernel's count.  Motion vector differences, DC differentials of all sizes, both picture types."""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    clip = D.wide_short_clip(mbw, 4, content, Q)
    n, mbs = clip.shape[0], mbw * 4
    _, d = orc.encode(clip, mbw, 4, pf, 7, 7, 3, Q, dump=True)
    enc = G.M.Mpeg2Encoder(7, 7, 3, Q)
    try:
        G.resident_encode(clip, mbw, 4, pf, 7, 7, 3, Q, enc=enc)
        aux = enc.debug_read(5, n * mbs * 16, np.uint32).reshape(n, mbs, 4).astype(np.int64)
    finally:
        enc.close()
    stored = (aux[:, :, 0] & 0xFFFF) + (aux[:, :, 0] >> 16) + (aux[:, :, 1] & 0xFFFF)
    want = D.slot_bits(d, mbw, pf)
    if content == "mix":
        assert d["mb_inter"][1:4].any() and not d["mb_inter"][1:4].all()        # both kinds in the P pictures
    assert stored.shape == want.shape and np.array_equal(stored, want), "first difference at macroblock %s" % (np.argwhere(stored != want)[:1],)


# ---- a wide fuzz ----
@pytest.mark.parametrize("seed", range(4))
def test_wide_fuzz(seed):
    """seeded: slice width 33 .. 128 macroblocks, 4 .. 6 rows, the dense generators and synth.clip, every VECTOR_LEVEL and Q_LEVEL;
    resident and port interface against the oracle; on a mismatch the stage comparison says where it starts"""
    import gpu_util as G
    from oracle import m2v_oracle_ctypes as orc
    rng = np.random.default_rng(7000 + seed)
    for case in range(5):
        mbw, ys16 = int(rng.integers(33, 129)), int(rng.integers(4, 7))
        content = str(rng.choice(["binary", "noise", "mix", "ramp", "checker", "synth"]))
        VL, Q = int(rng.integers(1, 4)), int(rng.integers(1, 5))
        pf = int(rng.choice([0, 1, 3, 255]))
        n = int(rng.integers(2, 7))
        bf = int(rng.choice([1, 2, 4, 96]))
        clip = D.make_clip(content, 16 * mbw, 16 * ys16, n, int(rng.integers(0, 1 << 20)), Q)
        tag = "seed %d case %d: %d x %d macroblocks, %s, n=%d pf=%d VL=%d Q=%d batch=%d" % (seed, case, mbw, ys16, content, n, pf, VL, Q, bf)
        want = orc.encode(clip, mbw, ys16, pf, 7, 7, VL, Q)
        got = G.resident_encode(clip, mbw, ys16, pf, 7, 7, VL, Q, batch_frames=bf)
        if got != want:                # (the debug build keeps the dumps of its last chunk: the stage comparison runs the clip as one chunk)
            pytest.fail(tag + " (crc %08x against %08x)\n" % (zlib.crc32(got), zlib.crc32(want))
                        + "\n".join(G.compare_stages(clip, mbw, ys16, pf, 7, 7, VL, Q)))
        enc = G.M.Mpeg2Encoder(7, 7, VL, Q)
        try:
            enc.set_option("batch_frames", bf)
            assert enc.encode(clip, mbw, ys16, pf) == want, tag + " (port interface)"
        finally:
            enc.close()
