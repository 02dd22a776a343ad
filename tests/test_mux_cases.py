"""CPU: the cases of tests/mux_cases.py reach what they are meant to reach - counted in the CPU muxers' output -, the device muxer's
arithmetic (csrc/m2v_mux_kernels.hpp, compiled with g++ and run unit by unit) reproduces m2vc_mux_ts / m2vc_mux_ps byte for byte on
every one of them, and m2v_mux_bound is never below the real size.  Byte equality only."""
import numpy as np
import pytest

import mux_cases as Q

M = Q.M


def ts_packets(ts):
    """-> [(pid, pusi, adaptation field bytes incl. the length byte, PCR flag)]"""
    assert len(ts) % 188 == 0
    out = []
    for k in range(0, len(ts), 188):
        p = ts[k:k + 188]
        assert p[0] == 0x47
        af = 1 + p[4] if (p[3] >> 4) & 2 else 0
        out.append(((p[1] & 0x1F) << 8 | p[2], bool(p[1] & 0x40), af, bool(af >= 2 and p[5] & 0x10), p[3] & 15))
    return out


def pes_shapes(ts):
    """the video PES packets of a transport stream -> [[adaptation field bytes of each of its packets]]"""
    pes = []
    for pid, pusi, af, pcr, cc in ts_packets(ts):
        if pid == 0x100:
            if pusi:
                assert pcr and af >= 8
                pes.append([])
            pes[-1].append(af)
    return pes


def ps_packs(ps):
    """-> [(pack bytes, has system header, has PTS, payload bytes)]"""
    out, p = [], 0
    while ps[p:p + 4] != b"\x00\x00\x01\xb9":
        assert ps[p:p + 4] == b"\x00\x00\x01\xba"
        q = p + 14
        sys = ps[q:q + 4] == b"\x00\x00\x01\xbb"
        if sys:
            q += 15
        assert ps[q:q + 4] == b"\x00\x00\x01\xe0"
        n = ps[q + 4] << 8 | ps[q + 5]
        pts = ps[q + 7] >> 6 == 2
        out.append((q + 6 + n - p, sys, pts, n - 3 - (5 if pts else 0)))
        p = q + 6 + n
    assert p + 4 == len(ps)
    return out


def test_ts_stuffing_shapes_are_reached():
    shapes = pes_shapes(Q.cpu_mux("ts", Q.cases()["ts_stuffing"]))
    last = [s[-1] for s in shapes if len(s) > 1]
    assert 0 in last, "184 bytes left: the last packet has no adaptation field"
    assert 1 in last, "183 left: adaptation_field_length = 0"
    assert 2 in last, "182 left"
    assert 183 in last, "1 byte left"
    single = [s[0] for s in shapes if len(s) == 1]
    assert 8 in single, "a PES packet of exactly 176 bytes: the PCR and nothing behind it"
    assert any(a > 8 for a in single), "a PES packet that fits its first packet: stuffing behind the PCR"


def test_ps_pack_shapes_are_reached():
    packs = ps_packs(Q.cpu_mux("ps", Q.cases()["ps_packs"]))
    assert packs[0][1] and packs[0][0] == 2048 and not any(p[1] for p in packs[1:]), "the system header, in the first pack, which is full"
    full_then_new = [a for a, b in zip(packs, packs[1:]) if a[0] == 2048 and a[2] and b[2]]
    assert len(full_then_new) >= 2, "a picture that ends exactly at its first pack's end"
    assert any(p[3] == 1 and not p[2] and p[0] == 24 for p in packs), "a picture one byte past a pack's end"
    assert any(a[0] == 2048 and not a[2] and b[2] for a, b in zip(packs, packs[1:])), "... and one that ends exactly at a later pack's end"
    assert any(p[2] and p[0] < 2048 for p in packs), "a picture smaller than a pack"


def test_rates_and_headers_are_reached():
    c = Q.cases()
    for code in range(1, 9):
        info, pics = Q.C.scan(c["rate%d" % code])
        assert info.frame_rate_code == code and info.pictures == 5
    # either side of the floor: 125 000 bytes/s = mux_rate 2500 in the pack header's units of 50 bytes/s
    def mux_rate(ps):
        return ps[10] << 14 | ps[11] << 6 | ps[12] >> 2
    assert mux_rate(Q.cpu_mux("ps", c["rate2"])) == 2500 and mux_rate(Q.cpu_mux("ps", c["fast"])) > 2500
    pk = ts_packets(Q.cpu_mux("ts", c["long"]))
    pat = [p for p in pk if p[0] == 0]
    pmt = [p for p in pk if p[0] == 0x1000]
    vid = [p for p in pk if p[0] == 0x100]
    assert len(pat) == len(pmt) > 16 and len(vid) > 16, "the continuity counters of all three PIDs wrap"
    assert [p[4] for p in pat] == [k & 15 for k in range(len(pat))] and [p[4] for p in vid] == [k & 15 for k in range(len(vid))]
    assert len([p for p in ts_packets(Q.cpu_mux("ts", c["fast"])) if p[0] == 0]) >= 1
    info, pics = Q.C.scan(c["long"])
    assert sum(1 for p in pics[1:] if c["long"][p.offset:p.offset + 4] == b"\x00\x00\x01\xb3") == 5, "repeated sequence headers open their access units"
    assert len(Q.C.scan(c["small"])[1]) == 300 and len(Q.C.scan(c["one"])[1]) == 1


def test_scan_boundaries_are_reached():
    T = Q.scan_tile()
    assert T % 1024 == 0, "a multiple of a wavefront's 64 x 16 bytes: a tile boundary is a lane and a wavefront boundary too"
    for k in range(4):
        es = Q.cases()["boundary%d" % k]
        assert 5 * T - 8 <= len(es) <= 5 * T + 64
        assert es[T - k:T - k + 4] == b"\x00\x00\x01\x00" and es[2 * T - k:2 * T - k + 4] == b"\x00\x00\x01\xb8"
        assert es[3 * T - k:3 * T - k + 4] == b"\x00\x00\x01\xb3" and es[5 * T - k:5 * T - k + 4] == b"\x00\x00\x01\xb7"
        info, pics = Q.C.scan(es)
        assert [p.offset for p in pics] == [34, T - k, 2 * T - k, 3 * T - k]


def test_error_cases_are_errors_for_the_cpu_muxers():
    for name, (es, status) in Q.error_cases().items():
        for kind in Q.KINDS:
            assert Q.cpu_mux(kind, es) == status, name


ALL = sorted(Q._cases())


@pytest.mark.parametrize("kind", Q.KINDS)
@pytest.mark.parametrize("name", ALL + ["oracle_" + k for k in Q.ORACLE_CLIPS])
def test_host_arithmetic_reproduces_the_cpu_muxers(name, kind):
    es = Q.oracle_clip(name[7:])[1] if name.startswith("oracle_") else Q.cases()[name]
    want = Q.cpu_mux(kind, es)
    assert isinstance(want, bytes)
    got, pictures = Q.host_mux(kind, es)
    assert isinstance(got, bytes), (name, got)
    if got != want:
        a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
        m = min(a.size, b.size)
        d = np.nonzero(a[:m] != b[:m])[0]
        raise AssertionError("%s %s: %d bytes, expected %d, first difference at %s" % (name, kind, a.size, b.size, d[0] if d.size else m))
    assert pictures == len(Q.C.scan(es)[1])
    assert M.mux_bound(kind, len(es), pictures) >= len(want), "m2v_mux_bound is below the real size"
    assert Q.host_lib().mux_host_bound(M.MUX_KINDS[kind], len(es), pictures) == M.mux_bound(kind, len(es), pictures)


@pytest.mark.parametrize("kind", Q.KINDS)
def test_host_arithmetic_at_every_misalignment_and_cap(kind):
    es = Q.cases()["rate4"]
    want = Q.cpu_mux(kind, es)
    for lead in range(16):
        assert Q.host_mux(kind, es, lead=lead)[0] == want, lead
    assert Q.host_mux(kind, es, cap=len(want))[0] == want and Q.host_mux(kind, es, cap=len(want) - 1)[0] == Q.OVERFLOW


@pytest.mark.parametrize("kind", Q.KINDS)
def test_host_arithmetic_refuses_the_error_cases(kind):
    for name, (es, status) in Q.error_cases().items():
        assert Q.host_mux(kind, es)[0] == status, name


def test_bound_and_layout():
    assert M.mux_bound(0, 1000, 3) == 0 and M.mux_bound(3, 1000, 3) == 0
    assert Q.layout([100, Q.SYNTAX, 33, 5], 200) == [(0, 100, 0), (128, 0, Q.SYNTAX), (128, 33, 0), (192, 5, 0)]
    assert Q.layout([100, 33, 5], 160) == [(0, 100, 0), (128, 0, Q.OVERFLOW), (128, 5, 0)]
