"""A writer of MPEG-2 transport and program streams for the demultiplexer's tests (m2vc_demux_ts / m2vc_demux_ps, m2v_demux_device), in the
manner of tests/dec_writer.py: every field is put bit by bit at the width ISO/IEC 13818-1 gives it (tables 2-2, 2-6, 2-21, 2-30, 2-33,
2-34, 2-38), nothing is taken from m2v_container.cpp or from what a demultiplexer computes.  The writers log what they write: per PES
packet of the video stream its elementary bytes and its stamp, the record a demultiplexer must answer, and - for a container written
broken on purpose - the verdict and the offset of the earliest packet or unit that breaks a rule.  tests/test_demux_cases.py asserts the
coverage it names from these logs.

The payload is not video: seeded bytes with 00 00 01 BA, 00 00 01 E0, 00 00 01 B9 and runs of 0x47 put in on purpose, and whole fake
pack headers and PES headers where a case asks for them."""
import numpy as np

ABSENT = 0xFFFFFFFFFFFFFFFF
OK, SYNTAX, OVERFLOW, NOSTREAM = 0, -2, -3, -4
NULL_PID = 0x1FFF


def crc32_mpeg(data):
    c = 0xFFFFFFFF
    for b in data:
        c ^= b << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7) & 0xFFFFFFFF if c & 0x80000000 else (c << 1) & 0xFFFFFFFF
    return c


class Bits:
    def __init__(self):
        self.v, self.n = 0, 0

    def put(self, value, width):
        assert 0 <= value < (1 << width), (value, width)
        self.v, self.n = self.v << width | value, self.n + width
        return self

    def bytes(self):
        assert self.n % 8 == 0
        return self.v.to_bytes(self.n // 8, "big")


def payload(rng, n):
    """n seeded bytes that look like structure wherever they can: start codes of packs, video packets and the end code, sync bytes"""
    b = bytearray(rng.randint(0, 256, size=n).astype(np.uint8).tobytes())
    for pat in (b"\x00\x00\x01\xba", b"\x00\x00\x01\xe0", b"\x00\x00\x01\xb9", b"\x47" * 5, b"\x00\x00\x01\xbb", b"\x00\x00\x01"):
        if n >= len(pat) and rng.randint(0, 3):
            at = rng.randint(0, n - len(pat) + 1)
            b[at:at + len(pat)] = pat
    return bytes(b)


def stamp_field(prefix, t, markers=(1, 1, 1)):
    """'xxxx' t[32..30] m t[29..15] m t[14..0] m"""
    return Bits().put(prefix, 4).put(t >> 30 & 7, 3).put(markers[0], 1).put(t >> 15 & 0x7FFF, 15).put(markers[1], 1).put(t & 0x7FFF, 15).put(markers[2], 1).bytes()


def pes_header(stream_id, length, pts=None, dts=None, stuffing=0, **broken):
    """packet_start_code_prefix .. PES_header_data_length and the header data: stamps, then stuffing bytes.  broken: a field's wrong value"""
    flags = 3 if dts is not None else 2 if pts is not None else 0
    data = b""
    if pts is not None:
        data += stamp_field(broken.get("pts_prefix", flags), pts, broken.get("pts_markers", (1, 1, 1)))
    if dts is not None:
        data += stamp_field(broken.get("dts_prefix", 1), dts, broken.get("dts_markers", (1, 1, 1)))
    data += b"\xff" * stuffing
    b = Bits().put(broken.get("prefix", 1), 24).put(stream_id, 8).put(length, 16)
    b.put(broken.get("marker", 2), 2).put(broken.get("scrambling", 0), 2).put(0, 1).put(1 if pts is not None else 0, 1).put(0, 1).put(0, 1)
    b.put(broken.get("flags", flags), 2).put(0, 6)
    b.put(broken.get("hl", len(data)), 8)
    return b.bytes() + data


def fake_structures(rng):
    """what a skipped packet may hold: a whole pack header, a video PES header with stamps, a transport packet header, an end code"""
    pack = Bits().put(0x000001BA, 32).put(1, 2).put(0, 3).put(1, 1).put(0, 15).put(1, 1).put(77, 15).put(1, 1).put(0, 9).put(1, 1).put(5000, 22).put(3, 2).put(0x1F, 5).put(0, 3).bytes()
    return pack + pes_header(0xE0, 40, pts=1234, dts=1000) + payload(rng, 31) + b"\x47\x41\x00\x10" + b"\x00\x00\x01\xb9" + pack


# ---------------------------------------------------------------------------------------------------------------------------------------
# transport stream
# ---------------------------------------------------------------------------------------------------------------------------------------
def ts_packet(pid, cc, data=b"", pusi=0, tei=0, tsc=0, di=0, sync=0x47, afc=None, afl=None):
    """table 2-2: sync_byte 8, transport_error_indicator 1, payload_unit_start_indicator 1, transport_priority 1, PID 13,
    transport_scrambling_control 2, adaptation_field_control 2, continuity_counter 4; an adaptation field (table 2-6: length 8,
    discontinuity_indicator 1, seven more flags, stuffing) sized so that `data` ends the packet"""
    n = len(data)
    assert n <= 184
    if afc is None:
        afc = 1 if n == 184 else 3 if n else 2
    out = Bits().put(sync, 8).put(tei, 1).put(pusi, 1).put(0, 1).put(pid, 13).put(tsc, 2).put(afc, 2).put(cc, 4).bytes()
    if n < 184:
        room = 184 - n
        out += bytes([room - 1 if afl is None else afl])
        if room >= 2:
            out += Bits().put(di, 1).put(0, 7).bytes() + b"\xff" * (room - 2)
    out += data
    assert len(out) == 188
    return out


def psi_section(table_id, id16, body, syntax=1, bad_crc=False):
    """table_id 8, section_syntax_indicator 1, '0' 1, reserved 2, section_length 12, id 16, reserved 2, version 5, current_next 1,
    section_number 8, last_section_number 8, body, CRC_32"""
    s = Bits().put(table_id, 8).put(syntax, 1).put(0, 1).put(3, 2).put(5 + len(body) + 4, 12).put(id16, 16).put(3, 2).put(0, 5).put(1, 1).put(0, 8).put(0, 8).bytes() + body
    c = crc32_mpeg(s) ^ (0x10 if bad_crc else 0)
    return s + c.to_bytes(4, "big")


def pat_section(programs, **kw):
    body = b"".join(Bits().put(pn, 16).put(7, 3).put(pid, 13).bytes() for pn, pid in programs)
    return psi_section(0, 1, body, **kw)


def pmt_section(program, pcr_pid, streams, program_info=b"", **kw):
    """streams: (stream_type, PID, ES_info bytes)"""
    body = Bits().put(7, 3).put(pcr_pid, 13).put(15, 4).put(len(program_info), 12).bytes() + program_info
    for st, pid, info in streams:
        body += Bits().put(st, 8).put(7, 3).put(pid, 13).put(15, 4).put(len(info), 12).bytes() + info
    return psi_section(2, program, body, **kw)


class TsWriter:
    """Packets in the order of the calls.  video_pid: what the demultiplexer must end up with; arg: what it is told (None: find it)."""

    def __init__(self, seed, video_pid=0x100, arg=None):
        self.rng = np.random.RandomState(seed)
        self.out = bytearray()
        self.video_pid, self.arg = video_pid, arg
        self.cc = {}
        self.es = bytearray()                 # the elementary stream a demultiplexer must return
        self.pes = []                         # per PES packet: dict(es=, es_offset=, pts=, dts=, src_offset=, head=)
        self.rec = dict(pes_packets=0, packets=0, discontinuities=0, skipped=0)
        self.started = False
        self.last_payload = False             # a video packet with a payload has been written
        self.errors = []                      # offsets of the packets written broken
        self.nostream = False
        self.log = dict(payload_lengths=[], hl=[], stuffed_headers=0, empty_pes=0, other_pids=set(), null=0, tei=0, di_gaps=0, plain_gaps=0,
                        wraps=0, leading=0, psi=[])

    # -- anything --
    def raw(self, packet):
        self.out += packet

    def _next_cc(self, pid, gap=0):
        c = (self.cc.get(pid, 15) + 1 + gap) & 15
        self.cc[pid] = c
        return c

    def psi(self, pid, section, pointer=0, broken=False, **kw):
        data = bytes([pointer]) + b"\xff" * pointer + section
        if not kw.pop("short", False):        # (short: an adaptation field in front instead of stuffing behind)
            data += b"\xff" * max(0, 184 - len(data))
        if broken:
            self.errors.append(len(self.out))
        self.log["psi"].append(pid)
        self.raw(ts_packet(pid, self._next_cc(pid), data[:184], pusi=1, **kw))

    def other(self, pid, n=184, pusi=0):
        """a packet of a PID that is not the video's: its payload is anything, a video PES header with PUSI set included"""
        assert pid != self.video_pid
        data = payload(self.rng, n)
        if pusi and n >= 19:
            data = pes_header(0xE0, 0, pts=99, dts=98) + data[19:]
        self.log["other_pids"].add(pid)
        self.raw(ts_packet(pid, self._next_cc(pid), data, pusi=pusi))

    def null(self):
        self.log["null"] += 1
        self.raw(ts_packet(NULL_PID, 0, b"\xff" * 184))

    def tei(self, pid=None):
        """a packet with transport_error_indicator: ignored whatever it holds (here: a PES start that would otherwise count)"""
        self.log["tei"] += 1
        pid = self.video_pid if pid is None else pid
        self.raw(ts_packet(pid, int(self.rng.randint(0, 16)), pes_header(0xE0, 0, pts=5) + payload(self.rng, 170), pusi=1, tei=1))

    # -- the video PID --
    def video(self, data, pusi=0, head=0, stamp=(ABSENT, ABSENT), gap=0, di=0, broken=False, **kw):
        """one packet: `data` = `head` bytes of PES header and elementary bytes.  gap: continuity_counter steps skipped (-1: a duplicate
        counter); broken: the packet breaks a rule (kw says which field)"""
        off = len(self.out)
        n = len(data)
        has_payload = bool(kw["afc"] & 1) if "afc" in kw else n > 0
        cc = self._next_cc(self.video_pid, gap) if has_payload else self.cc.get(self.video_pid, 0)
        self.raw(ts_packet(self.video_pid, cc, data, pusi=pusi, di=di, **kw))
        if broken:
            self.errors.append(off)
            return
        self.rec["packets"] += 1
        self.log["payload_lengths"].append(n)
        if has_payload:
            if self.last_payload and gap:
                self.log["di_gaps" if di else "plain_gaps"] += 1
                if not di:
                    self.rec["discontinuities"] += 1
            if self.last_payload and cc == 0 and not gap:
                self.log["wraps"] += 1
            self.last_payload = True
        if pusi:
            self.started = True
            self.pes.append(dict(es=bytes(data[head:]), es_offset=len(self.es), pts=stamp[0], dts=stamp[1], src_offset=off + 188 - n, head=head))
            self.rec["pes_packets"] += 1
            self.log["hl"].append(head - 9)
            if n == head:
                self.log["empty_pes"] += 1
        if not self.started:
            self.rec["skipped"] += 1
            self.log["leading"] += 1
            return
        self.es += data[head:]

    def pes_packet(self, nbytes, pts=None, dts=None, stuffing=0, sizes=(), gap=0, di=0, stream_id=0xE0):
        """a PES packet of nbytes elementary bytes: the first packet takes sizes[0] bytes of header and payload (default: what fits), the
        next sizes[1] .. (0: an adaptation field only), the rest 184 each"""
        head = pes_header(stream_id, 0, pts, dts, stuffing)
        if stuffing:
            self.log["stuffed_headers"] += 1
        data = head + payload(self.rng, nbytes)
        sizes = list(sizes)
        first = sizes.pop(0) if sizes else min(184, len(data))
        assert len(head) <= first <= min(184, len(data))
        stamp = (ABSENT if pts is None else pts, ABSENT if dts is None else dts)
        self.video(data[:first], pusi=1, head=len(head), stamp=stamp, gap=gap, di=di)
        at = first
        while at < len(data) or sizes:
            k = sizes.pop(0) if sizes else min(184, len(data) - at)
            self.video(data[at:at + k])
            at += k
        assert at == len(data)

    def continuation(self, n):
        """a packet of the video PID without a PES start"""
        self.video(payload(self.rng, n))

    def expect(self):
        """-> dict(status, err_offset, es, stamps [(es_offset, pts, dts, src_offset)], record)"""
        n = len(self.out)
        errors = list(self.errors)
        if n == 0 or n % 188:
            errors.append(n // 188 * 188)
        if errors:
            return dict(status=SYNTAX, err_offset=min(errors), es=b"", stamps=[], record=None)
        if self.nostream or not self.pes:
            return dict(status=NOSTREAM, err_offset=0, es=b"", stamps=[], record=None)
        rec = dict(self.rec, out_bytes=len(self.es), stream=self.video_pid)
        return dict(status=OK, err_offset=0, es=bytes(self.es), stamps=[(p["es_offset"], p["pts"], p["dts"], p["src_offset"]) for p in self.pes],
                    record=rec)

    def bytes(self):
        return bytes(self.out)


# ---------------------------------------------------------------------------------------------------------------------------------------
# program stream
# ---------------------------------------------------------------------------------------------------------------------------------------
class PsWriter:
    """Units in the order of the calls.  arg: the stream_id the demultiplexer is told (None: the first video packet's)."""

    def __init__(self, seed, arg=None):
        self.rng = np.random.RandomState(seed)
        self.out = bytearray()
        self.arg, self.sel = arg, arg
        self.es = bytearray()
        self.pes = []
        self.rec = dict(pes_packets=0, packets=0, discontinuities=0, skipped=0)
        self.errors = []
        self.ended = False
        self.log = dict(pack_stuffing=[], units=[], unit_starts=[], system_headers=0, fake=0, hl=[], end_zeros=None, video_ids=set())

    def _unit(self, b, broken=False):
        if broken:
            self.errors.append(len(self.out))
        self.log["unit_starts"].append(len(self.out))
        self.out += b

    def pack(self, stuffing=0, scr=0, rate=25000, broken=False, **bad):
        """table 2-33: pack_start_code 32, '01', SCR 3 m 15 m 15 m, extension 9 m, program_mux_rate 22 mm, reserved 5, pack_stuffing_length 3"""
        base, ext = scr // 300, scr % 300
        m = [bad.get("m%d" % k, 1) for k in range(5)]
        b = Bits().put(0x000001BA, 32).put(bad.get("two", 1), 2).put(base >> 30 & 7, 3).put(m[0], 1).put(base >> 15 & 0x7FFF, 15).put(m[1], 1)
        b.put(base & 0x7FFF, 15).put(m[2], 1).put(ext, 9).put(m[3], 1).put(rate, 22).put(bad.get("mm", 3), 2).put(0x1F, 5).put(stuffing, 3)
        self._unit(b.bytes() + b"\xff" * stuffing, broken)
        if not broken:
            self.rec["packets"] += 1
            self.log["pack_stuffing"].append(stuffing)

    def pack_mpeg1(self):
        """ISO/IEC 11172-1: '0010' SCR 3 m 15 m 15 m, m mux_rate 22 m: 12 bytes"""
        b = Bits().put(0x000001BA, 32).put(2, 4).put(0, 3).put(1, 1).put(0, 15).put(1, 1).put(9, 15).put(1, 1).put(1, 1).put(5000, 22).put(1, 1)
        self._unit(b.bytes(), True)

    def unit(self, stream_id, data, broken=False, length=None):
        """any unit with a length field: start code, PES_packet_length 16, the bytes"""
        b = Bits().put(1, 24).put(stream_id, 8).put(len(data) if length is None else length, 16).bytes() + data
        self._unit(b, broken)
        if not broken:
            self.rec["skipped"] += 1
            self.log["units"].append(stream_id)

    def system_header(self, video_ids=(0xE0,)):
        """table 2-34: m rate_bound 22 m, audio_bound 6, fixed 1, CSPS 1, audio_lock 1, video_lock 1, m, video_bound 5, restriction 1,
        reserved 7; per stream: stream_id 8, '11', scale 1, size 13"""
        b = Bits().put(1, 1).put(25000, 22).put(1, 1).put(1, 6).put(0, 1).put(0, 1).put(0, 1).put(0, 1).put(1, 1).put(len(video_ids), 5).put(0, 1).put(0x7F, 7)
        for sid in video_ids:
            b.put(sid, 8).put(3, 2).put(1, 1).put(46, 13)
        self.log["system_headers"] += 1
        self.unit(0xBB, b.bytes())

    def fake(self, stream_id):
        """a skipped packet (padding BE, private BD / BF, audio C0 .., a stream map BC) whose bytes hold whole pack and video PES headers"""
        self.log["fake"] += 1
        self.unit(stream_id, fake_structures(self.rng) + payload(self.rng, int(self.rng.randint(0, 90))))

    def filler(self, n, stream_id=0xBE):
        """n bytes in all (n >= 6), skipped"""
        self.unit(stream_id, payload(self.rng, n - 6))

    def pes_packet(self, stream_id, nbytes, pts=None, dts=None, stuffing=0, broken=False, **bad):
        self.log["video_ids"].add(stream_id)
        if self.sel is None:
            self.sel = stream_id
        if stream_id != self.sel:
            head = pes_header(stream_id, 0, pts, dts, stuffing)
            self.unit(stream_id, head[6:] + payload(self.rng, nbytes))
            return
        es = payload(self.rng, nbytes)
        length = bad.pop("length", None)
        head = pes_header(stream_id, 0, pts, dts, stuffing, **bad)
        L = len(head) - 6 + nbytes if length is None else length
        head = head[:4] + Bits().put(L, 16).bytes() + head[6:]
        off = len(self.out)
        self._unit(head + es, broken)
        if broken:
            return
        self.pes.append(dict(es=es, es_offset=len(self.es), pts=ABSENT if pts is None else pts, dts=ABSENT if dts is None else dts, src_offset=off,
                             head=len(head)))
        self.rec["pes_packets"] += 1
        self.log["hl"].append(len(head) - 9)
        self.es += es

    def end(self, zeros=0, tail=b""):
        self._unit(b"\x00\x00\x01\xb9")
        self.log["end_zeros"] = zeros
        self.out += bytes(zeros)
        if tail:
            self.errors.append(len(self.out) + next(k for k, v in enumerate(tail) if v))
            self.out += tail

    def garbage(self, b):
        """bytes where a unit must start"""
        self._unit(b, True)

    def expect(self):
        if self.errors:
            return dict(status=SYNTAX, err_offset=min(self.errors), es=b"", stamps=[], record=None)
        if not self.pes:
            return dict(status=NOSTREAM, err_offset=0, es=b"", stamps=[], record=None)
        rec = dict(self.rec, out_bytes=len(self.es), stream=self.sel)
        return dict(status=OK, err_offset=0, es=bytes(self.es), stamps=[(p["es_offset"], p["pts"], p["dts"], p["src_offset"]) for p in self.pes], record=rec)

    def bytes(self):
        return bytes(self.out)
