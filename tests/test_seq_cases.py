"""What the cases of tests/seq_cases.py reach, shown on the CPU: the expectations of tests/test_gpu_sequences.py are legal streams of
the right pictures, their offsets are aligned, the clips hit the remainders the final-word rule turns on, and the chosen chunk grids cut
the lists in every way the scan has to handle.  No GPU, nothing of the library's device code."""
import numpy as np
import pytest

import seq_cases as Q

G, M = Q.G, Q.M


def all_cases():
    out = [Q.parity(n) for n in Q.PARITY] + [Q.remainder_case(), Q.comp()]
    return out


def test_every_stream_is_whole_words_and_offsets_are_aligned():
    for c in all_cases():
        s = Q.streams(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
        data, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
        assert all(len(x) % 32 == 0 for x in s)
        assert off[0] == 0 and all(o % 32 == 0 for o in off) and off[-1] == len(data)
        for b, x in enumerate(s):
            B = Q.front_bytes(x)
            assert len(x) == ((B + 4) // 32 + 1) * 32                # the module's final-word rule, applied to the clip alone
            assert data[off[b]:off[b + 1]] == x and x[:4] == b"\x00\x00\x01\xb3"
        r = Q.records(c["lengths"], off, c["pf"])
        assert r["first_frame"].tolist() == np.cumsum([0] + c["lengths"])[:-1].tolist()
        assert int(r["offset"][-1] + r["bytes"][-1]) == len(data)


@pytest.mark.parametrize("name", ["mixed_pf2", "fives_pf4"])
def test_every_piece_decodes_to_the_oracles_reconstruction(name):
    c = Q.parity(name)
    data, off = Q.expected(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
    for b, clip in enumerate(Q.split(c["frames"], c["lengths"])):
        d = M.decoder.decode(data[off[b]:off[b + 1]], quirks=True)       # (the module's loop, which the oracle's dump holds)
        rec = G.encoded(clip, c["W"], c["H"], c["pf"], 2)[1]["recon"]
        assert len(d.frames) == len(clip)
        assert [p["type"] for p in d.pictures] == [1 if k % (c["pf"] + 1) == 0 else 2 for k in range(len(clip))]
        for k, f in enumerate(d.frames):
            assert np.array_equal(np.concatenate([p.reshape(-1) for p in f]), rec[k]), (b, k)


def test_remainders():
    """0, 27, 28, 29 and 31 bytes over a whole word in front of the end code; 28 is the one where a whole extra zero word leaves"""
    c = Q.remainder_case()
    s = Q.streams(c["frames"], c["lengths"], c["W"], c["H"], c["pf"])
    got = [Q.front_bytes(x) % 32 for x in s]
    assert got == c["remainders"] and set(got) == {0, 27, 28, 29, 31}
    for x, r in zip(s, got):
        assert len(x) - Q.front_bytes(x) == (36 if r == 28 else 32 - (r + 4) % 32 + 4)
    # the sequences of the other cases add more remainders; the five above are the ones the rule turns on
    assert len({Q.front_bytes(x) % 32 for c2 in all_cases() for x in Q.streams(c2["frames"], c2["lengths"], c2["W"], c2["H"], c2["pf"])}) > 5


def test_chunk_grids_reach_every_situation():
    seen = set()
    for chunk in Q.CHUNKS:
        seen |= Q.situations(Q.MIXED, chunk)
    assert seen == Q.ALL_SITUATIONS
    assert "every_frame_a_sequence" in Q.situations(Q.MIXED, 4) and "spans_three_chunks" in Q.situations(Q.MIXED, 4)
    assert "ends_on_chunk_last" in Q.situations(Q.MIXED, 4) and "ends_on_chunk_first" in Q.situations(Q.MIXED, 5)
    assert Q.situations(Q.MIXED, 96) <= {"one_frame", "ends_inside"}            # one chunk holds the batch
    assert "ends_on_chunk_last" in Q.situations(Q.FIVES, 5) and "spans_three_chunks" not in Q.situations(Q.FIVES, 5)


def test_trip_cases_pass_the_scans_thresholds():
    rows = 64 // 16
    below, above = Q.TRIP_COUNTS["below"], Q.TRIP_COUNTS["above_all"]
    assert below * rows == 1024                                                 # one item a thread, none over
    assert above * rows > 4096 and -(-above * rows // 1024) > 4 and above > 1024    # past the cached items; two sequences a thread
    c = Q.trip_case("below")
    assert len(c["stream"]) == c["offsets"][-1] and len(set(np.diff(c["offsets"]).tolist())) > 1


def test_python_argument_checks():
    assert M.check_sequences([1, 2, 3], 6) == [1, 2, 3]
    with pytest.raises(ValueError):
        M.check_sequences([1, 2, 3], 7)             # the sum is not the call's frames
    with pytest.raises(ValueError):
        M.check_sequences([3, 0, 3], 6)             # an entry of 0
    assert M.SEQUENCE_STAT_DTYPE.itemsize == 32 == __import__("ctypes").sizeof(M.SequenceStat)
