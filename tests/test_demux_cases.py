"""CPU: the demultiplexers' specification (m2vc_demux_ts / m2vc_demux_ps of libm2v_container.so) and the device demultiplexer's host build
(csrc/m2v_demux_kernels.hpp behind tools/demux_host.hpp) on the containers of tests/demux_cases.py.  Three witnesses: the muxers of the
same library with the Python demultiplexers of tests/test_container.py, the log of tests/demux_writer.py - written from the standard's
field widths, not from the C++ - and, for the host build, the specification itself.  What the cases reach is asserted from the writer's
log.  tests/test_gpu_demux.py runs the same containers on the device."""
import os
import subprocess

import pytest

import demux_cases as DC
import demux_writer as W
import mux_cases as Q
import test_container as TC

M, C = DC.M, DC.C
CSRC = os.path.join(os.path.dirname(os.path.abspath(M.__file__)), "csrc")


def same(a, b, what):
    """two answers agree in every part"""
    for f in ("status", "err_offset", "record", "stamps"):
        assert a[f] == b[f], (what, f, a[f] if f != "stamps" else len(a[f]), b[f] if f != "stamps" else len(b[f]))
    assert a["es"] == b["es"], (what, "bytes", len(a["es"]), len(b["es"]))


def matches_log(got, expect, what):
    assert (got["status"], got["err_offset"]) == (expect["status"], expect["err_offset"]), (what, got["status"], got["err_offset"], expect["status"], expect["err_offset"])
    if expect["status"] == DC.OK:
        assert got["es"] == expect["es"] and got["stamps"] == expect["stamps"] and got["record"] == expect["record"], (what, got["record"], expect["record"])
    else:
        assert got["es"] == b"" and got["stamps"] == [] and not any(got["record"].values()), what


def test_headers_and_exports():
    h = open(os.path.join(DC.ROOT, "include", "m2v_mi355x.h")).read()
    for word in ("m2v_demux_device", "m2v_demux_report", "m2v_demux_bound", "m2v_demux_scan_tile", "M2V_DEMUX_SYNTAX = -2", "M2V_DEMUX_OVERFLOW = -3",
                 "M2V_DEMUX_NOSTREAM = -4", "m2v_demux_stat", "m2v_demux_stamp"):
        assert word in h, word
    c = open(os.path.join(DC.ROOT, "include", "m2v_container.h")).read()
    for word in ("m2vc_demux_ts", "m2vc_demux_ps", "m2vc_stamp", "m2vc_demux_info", "M2VC_E_NOSTREAM", "DUPLICATE"):
        assert word in c, word
    for name in ("m2v_demux_bound", "m2v_demux_device", "m2v_demux_report", "m2v_demux_scan_tile"):
        assert name in M.EXPORTS and hasattr(M.lib(), name)
    assert M.DEMUX_STAT_DTYPE.itemsize == 64 and M.DEMUX_STAMP_DTYPE.itemsize == 32
    assert M.demux_scan_tile() % 188 == 0 and M.demux_bound([1, 32, 33]) == 32 + 32 + 64 and M.demux_bound([]) == 0


# ---- the inverse of the muxers of the same library ----
@pytest.mark.parametrize("name", sorted(Q.cases()))
def test_demux_of_mux_is_the_stream(name):
    es = Q.cases()[name]
    info, pics = C.scan(es)
    ts, ps = Q.cpu_mux("ts", es), Q.cpu_mux("ps", es)
    got, stamps, rec = C.demux_ts(ts)
    ref, pts, _, _ = TC.demux_ts(ts)
    assert got == es[:info.bytes] == ref
    assert [s.pts for s in stamps] == pts and all(s.dts == C.ABSENT for s in stamps)
    assert rec.pes_packets == len(pts) == len(pics) and rec.stream == 0x100 and rec.discontinuities == 0 and rec.skipped == 0
    assert rec.packets == sum(1 for k in range(0, len(ts), 188) if (ts[k + 1] & 0x1F) << 8 | ts[k + 2] == 0x100)
    assert C.demux_ts(ts, pid=0x100)[0] == got
    got, stamps, rec = C.demux_ps(ps)
    ref, marks, scrs, _ = TC.demux_ps(ps)
    assert got == es[:info.bytes] == ref
    assert [(s.es_offset, s.pts) for s in stamps if s.pts != C.ABSENT] == marks
    assert rec.pes_packets == len(scrs) == rec.packets and rec.stream == 0xE0 and rec.skipped == 1      # (the system header)
    for kind, box in (("ts", ts), ("ps", ps)):
        same(DC.host(kind, box, lead=len(es) & 15), DC.cpu(kind, box), name)


# ---- the written cases ----
@pytest.mark.parametrize("name", sorted(DC.cases()))
def test_written_case(name):
    c = DC.cases()[name]
    got = DC.cpu(c["kind"], c["data"], c["arg"])
    matches_log(got, c["expect"], name)
    for lead in (0, 9):
        same(DC.host(c["kind"], c["data"], c["arg"], lead=lead), got, name)
    if c["arg"] is None:                               # naming the stream the container's tables name changes nothing
        same(DC.cpu(c["kind"], c["data"], c["expect"]["record"]["stream"]), got, name)


@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_written_big(kind):
    c = DC.big(kind)
    got = DC.cpu(kind, c["data"], c["arg"])
    matches_log(got, c["expect"], kind)
    same(DC.host(kind, c["data"], c["arg"], lead=3), got, kind)
    assert len(c["data"]) > 2 << 20 and len(got["stamps"]) >= 40


def test_coverage_transport():
    cs = DC.cases()
    tile = DC.scan_tile() // 188
    counts = sorted(len(c["data"]) // 188 for n, c in cs.items() if n.startswith("ts_n"))
    assert counts[:6] == [1, 63, 64, 65, 256, 257] and counts[6] > tile
    assert all(c["log"]["psi"] == [] and c["arg"] is not None for n, c in cs.items() if n.startswith("ts_n"))      # no PAT, the PID given
    c = cs["ts_shapes"]
    L = c["log"]
    assert {0, 1, 183, 184} <= set(L["payload_lengths"])
    assert {0, 5, 10} <= set(L["hl"]) and L["stuffed_headers"] >= 2 and max(L["hl"]) > 10
    assert L["empty_pes"] >= 1                         # a PES header that ends with its packet
    assert {0x1E0, 0x300} <= L["other_pids"] and L["null"] >= 2 and L["tei"] >= 2
    assert L["leading"] >= 3 and c["expect"]["record"]["skipped"] == L["leading"]
    assert L["psi"].count(0) >= 2 and 0x1000 in L["psi"] and 0x1001 in L["psi"]
    assert sum(1 for pn, _ in DC.PAT if pn) >= 2 and DC.PAT[0][0] == 0      # several programs, the first entry the network's
    assert L["wraps"] >= 1 and L["plain_gaps"] >= 2 and L["di_gaps"] >= 1
    assert c["expect"]["record"]["discontinuities"] == L["plain_gaps"]
    stamps = c["expect"]["stamps"]
    assert any(p == W.ABSENT for _, p, _, _ in stamps) and any(d != W.ABSENT for _, _, d, _ in stamps) and any(p != W.ABSENT and d == W.ABSENT for _, p, d, _ in stamps)
    # the first packets are the video PID's, in front of PAT and PMT
    assert (c["data"][1] & 0x1F) << 8 | c["data"][2] == 0x1E1 and c["log"]["psi"][0] == 0


def test_coverage_program():
    cs = DC.cases()
    L = cs["ps_shapes"]["log"]
    assert sorted(L["pack_stuffing"]) == list(range(8)) and L["system_headers"] == 1
    assert L["fake"] >= 5 and {0xBC, 0xBE, 0xBD, 0xBF, 0xC0} <= set(L["units"])
    assert {0, 5, 10} <= set(L["hl"]) and 9 in L["hl"] and L["end_zeros"] == 37
    assert cs["ps_no_end"]["log"]["end_zeros"] is None and not cs["ps_no_end"]["data"].endswith(b"\x00\x00\x01\xb9")
    two = cs["ps_second_id"]
    assert two["log"]["video_ids"] == {0xE0, 0xE1} and two["arg"] == 0xE1 and two["expect"]["record"]["stream"] == 0xE1
    assert cs["ps_shapes"]["expect"]["record"]["stream"] == 0xE0 and two["expect"]["es"] != cs["ps_shapes"]["expect"]["es"]
    T = DC.scan_tile()
    for k in range(5):                                 # a unit start k bytes in front of every multiple of the tile: the code straddles it for k = 1, 2, 3
        c = cs["ps_tile%d" % k]
        assert len(c["data"]) > 2 * T and {T - k, 2 * T - k} <= set(c["log"]["unit_starts"])
        assert c["data"][T - k:T - k + 4] == b"\x00\x00\x01\xe0"
    assert len(cs["ps_many_units"]["log"]["unit_starts"]) > 4096
    # payloads emulate structure: whole pack headers, video PES headers, end codes and sync bytes inside what is carried
    es = cs["ps_shapes"]["expect"]["es"] + cs["ts_shapes"]["expect"]["es"] + DC.big("ps")["expect"]["es"][:1 << 16]
    for pat in (b"\x00\x00\x01\xba", b"\x00\x00\x01\xe0", b"\x00\x00\x01\xb9", b"\x47" * 5):
        assert pat in es, pat


# ---- refusals ----
TS_RULES = ("length", "empty", "sync", "pat_table_id", "pat_syntax_indicator", "pat_crc", "pat_crosses", "pat_adaptation_183", "pat_no_program", "no_pat", "no_pmt",
            "pmt_crc", "pmt_program", "pmt_table_id", "pmt_info_length", "pmt_no_video", "scrambling_control", "adaptation_control_0", "adaptation_only_182",
            "adaptation_3_length_183", "pes_prefix", "pes_stream_id", "pes_marker_10", "pes_scrambling", "pes_flags_1", "pes_pts_short", "pes_pts_prefix",
            "pes_pts_marker", "pes_dts_short", "pes_dts_prefix", "pes_dts_marker", "pes_crosses_packet", "pes_under_9", "pes_start_without_payload", "no_start",
            "two_video_first", "two_sync_first")
PS_RULES = ("prefix", "code_b3", "code_b8", "mpeg1_pack", "pack_two", "pack_m0", "pack_m1", "pack_m2", "pack_m3", "pack_mm", "pes_length_0", "pes_length_2",
            "pes_hl_past_length", "pes_flags_1", "pes_marker_10", "pes_scrambling", "pes_pts_prefix", "pes_pts_marker", "pes_dts_prefix", "pes_dts_short",
            "pack_stuffing_cut", "pack_cut", "unit_past_end", "unit_cut", "code_cut", "after_end", "id_absent", "no_video", "empty", "two")
NOSTREAM = {"ts:pat_no_program", "ts:no_pat", "ts:no_pmt", "ts:pmt_no_video", "ts:no_start", "ps:id_absent", "ps:no_video", "ps:empty"}


def test_every_rule_has_its_refusal():
    r = DC.refusals()
    assert sorted(r) == sorted(["ts:" + n for n in TS_RULES] + ["ps:" + n for n in PS_RULES])
    assert {n for n, c in r.items() if c["expect"]["status"] == DC.NOSTREAM} == NOSTREAM
    # the offsets are the writer's: where it wrote the broken packet or unit, behind a valid start (so not 0) except for the empty input
    assert all(c["expect"]["err_offset"] > 0 for n, c in r.items() if c["expect"]["status"] == DC.SYNTAX and n not in ("ts:empty",) and not n.startswith("ts:pat_"))
    for n in ("ts:two_video_first", "ts:two_sync_first", "ps:two"):
        assert r[n]["expect"]["status"] == DC.SYNTAX


@pytest.mark.parametrize("name", ["ts:" + n for n in TS_RULES] + ["ps:" + n for n in PS_RULES])
def test_refusal(name):
    c = DC.refusals()[name]
    got = DC.cpu(c["kind"], c["data"], c["arg"])
    matches_log(got, c["expect"], name)
    same(DC.host(c["kind"], c["data"], c["arg"], lead=5), got, name)


# ---- capacities ----
@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_capacities(kind):
    c = DC.cases()[kind + "_shapes"]
    full = DC.cpu(kind, c["data"], c["arg"])
    n, pes = len(full["es"]), len(full["stamps"])
    short = DC.cpu(kind, c["data"], c["arg"], cap=n - 1)
    assert short["status"] == DC.OVERFLOW and short["record"]["out_bytes"] == n and short["es"] == b""
    few = DC.cpu(kind, c["data"], c["arg"], stamp_cap=pes - 2)
    assert few["status"] == DC.OK and few["es"] == full["es"] and few["stamps"] == full["stamps"][:pes - 2] and few["record"] == full["record"]
    h = DC.host(kind, c["data"], c["arg"], cap=n - 1)
    assert h["status"] == DC.OVERFLOW and h["es"] == b"" and not any(h["record"].values())
    h = DC.host(kind, c["data"], c["arg"], cap=n, stamp_cap=pes - 2)
    assert h["es"] == full["es"] and h["stamps"] == full["stamps"][:pes - 2] and h["record"] == full["record"]
    info = C.DemuxInfo()
    assert C.lib().m2vc_demux_ts(c["data"], len(c["data"]), 0x2000, None, 0, None, 0, info) == C.E_PARAM
    assert C.lib().m2vc_demux_ps(c["data"], len(c["data"]), 0xDF, None, 0, None, 0, info) == C.E_PARAM
    assert C.lib().m2vc_demux_ps(c["data"], len(c["data"]), -1, None, 0, None, 0, None) == C.E_PARAM


# ---- altered containers ----
@pytest.mark.parametrize("kind", ["ts", "ps"])
def test_altered_containers(kind):
    base, first = DC.alter_base(kind)
    ref = DC.cpu(kind, base["data"], base["arg"])
    matches_log(ref, base["expect"], kind)
    alts = DC.altered(kind)
    assert len(alts) == 8 * first + 500 and first == (376 if kind == "ts" else base["log"]["unit_starts"][5])
    changed = refused = 0
    for k, a in enumerate(alts):
        got = DC.cpu(kind, a, base["arg"])
        same(DC.host(kind, a, base["arg"], lead=k & 15), got, "%s altered %d" % (kind, k))
        refused += got["status"] != DC.OK
        changed += got["status"] == DC.OK and got["es"] != ref["es"]
    # a condition on the cases, met by the specification alone: neither branch is tested on a handful only
    assert 10 * changed >= len(alts) and 10 * refused >= len(alts), (changed, refused, len(alts))


# ---- one textual change at a time in a copy of csrc/m2v_demux_kernels.hpp: each is caught by a named case ----
MUTANTS = (
    ("pts_needs_5", "hl < (flags == 3 ? 10u : 5u)", "hl < (flags == 3 ? 10u : 4u)", "ts:pes_pts_short"),
    ("adaptation_182", "ok = p[4] <= 182;", "ok = p[4] <= 183;", "ts:adaptation_3_length_183"),
    ("adaptation_only_183", "ok = p[4] == 183;", "ok = p[4] >= 182;", "ts:adaptation_only_182"),
    ("counter_mod_16", "((last_cc + 1) & 15u)", "((last_cc + 1) & 31u)", "ts_shapes"),
    ("indicator_ignored", " && !(word & 16u)", "", "ts_shapes"),
    ("stamp_middle_shift", "(uint64_t)(b[2] >> 1) << 15", "(uint64_t)(b[2] >> 1) << 14", "ts_shapes"),
    ("transport_error_counts", "if ((p[1] & 0x80) || ts_pid(p) != pid) return k;", "if (ts_pid(p) != pid) return k;", "ts_shapes"),
    ("leading_bytes_kept", "out += T.bytes - T.bytes_pre;", "out += T.bytes;", "ts_shapes"),
    ("first_video_entry", "if (s[i] == 1 || s[i] == 2)", "if (s[i] == 2 || s[i] == 3)", "ts_shapes"),
    ("pack_stuffing", "p += 14u + (h[9] & 7);", "p += 14u;", "ps_shapes"),
    ("bytes_after_end", "if (src[q]) { S.err = q; break; }", "if (src[q] & 0xF0) { S.err = q; break; }", "ps:after_end"),
)


def _named(name):
    return DC.refusals()[name] if ":" in name else DC.cases()[name]


def _agrees(lib, c):
    got, want = DC.host(c["kind"], c["data"], c["arg"], lead=7, lib=lib), DC.cpu(c["kind"], c["data"], c["arg"])
    return all(got[f] == want[f] for f in ("status", "err_offset", "es", "stamps", "record"))


@pytest.mark.parametrize("name,old,new,case", MUTANTS, ids=[m[0] for m in MUTANTS])
def test_cases_catch_mutants(tmp_path, name, old, new, case):
    text = open(os.path.join(CSRC, "m2v_demux_kernels.hpp")).read()
    assert text.count(old) == 1, "the line this mutant changes is not there (once)"
    (tmp_path / "m2v_demux_kernels.hpp").write_text(text.replace(old, new))
    lib = DC.build_host(str(tmp_path))
    assert _agrees(DC.host_lib(), _named(case))
    assert not _agrees(lib, _named(case)), "mutant %s slipped past %s" % (name, case)


# ---- the host build under the sanitizers, as a program of its own ----
def test_standalone_sanitizer_program(tmp_path):
    items = [(c["kind"], c["arg"], c["data"]) for _, c in sorted(DC.cases().items())]
    items += [(c["kind"], c["arg"], c["data"]) for _, c in sorted(DC.refusals().items())]
    items += [(kind, DC.alter_arg(kind), a) for kind in ("ts", "ps") for a in DC.altered(kind)]
    items += [(kind, None, b) for kind in ("ts", "ps") for b in (b"", b"\x47", b"\x00\x00\x01", b"\x00\x00\x01\xba", bytes(188), b"\x47" * 188, b"\x00\x00\x01\xe0\xff\xff")]
    items += [(kind, DC.big(kind)["arg"], DC.big(kind)["data"]) for kind in ("ts", "ps")]
    path = tmp_path / "containers.bin"
    path.write_bytes(DC.pack_containers(items))
    exe = str(tmp_path / "demux_host_check")
    # the sanitizers' runtimes linked in: the program starts with whatever environment the test has
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", "-I", CSRC, "-I", os.path.join(DC.ROOT, "tools"), "-o", exe,
                           os.path.join(DC.ROOT, "tools", "demux_host_check.cpp")])
    p = subprocess.run([exe, str(path)], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert p.returncode == 0, p.stderr.decode()[-2000:]
    lines = p.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(items)
    # the program's verdicts are the specification's
    for k in list(range(0, len(items), 97)) + [len(items) - 1, len(items) - 2]:
        kind, arg, data = items[k]
        want = DC.cpu(kind, data, arg)
        assert [int(v) for v in lines[k].split()[:5]] == [k, want["status"], want["err_offset"], len(want["es"]), len(want["stamps"])], k
