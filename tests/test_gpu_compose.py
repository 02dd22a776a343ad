"""-m gpu: the settings of a resident call in combination, against the one model of tests/compose_cases.py.  Every comparison is byte for
byte or integer for integer (compose_cases.check): the elementary stream, the five reports, the reconstruction buffer and every
container with its record; every output buffer is filled with a sentinel first and nothing outside the reported ranges may change.
One case per row of pairs() on a fresh handle, the maximal sets blocking and as begin / end, a session of a dozen calls on ONE handle
that change several settings and the geometry at once, two handles taking turns, every refused pair, the port path in a covering array
of its own, and encode_tensor / encode_batch with a maximal set as keywords.  tests/test_compose_cases.py shows what the rows cover and
that the comparison can fail.  Nothing is larger than 112 x 80 and 12 frames.

Measured on one MI355X: 103 cases in 3.8 s (the slowest, the first of the file, 0.21 s)."""
import numpy as np
import pytest

import compose_cases as C

pytestmark = pytest.mark.gpu
M, D, G, X = C.M, C.D, C.G, C.X
E_STATE = -4


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, dtype=np.uint8, order="C")).to("cuda:0")


def filled(n, value):
    import torch
    return torch.full((n,), value, dtype=torch.uint8, device="cuda:0")


def resolved(c):
    """the values a handle holds for a call's settings"""
    w, h, header = c["geom"]
    return dict(size=(w, h, header) if header else None, conformant=c["conformant"], stats=c["stats"], chunk=c["chunk"], split=c["split"],
                levels=C.levels_of(c), cap=C.cap_of(c), starts=C.starts_of(c), cut=C.cut_of(c),
                desc=tuple(sorted(C.desc_of(c).items())) if c["desc"] else None, seqs=C.lengths_of(c), recon=c["recon"], mux=c["mux"])


NOTHING = resolved(C.OFF)


class Handle:
    """an encoder and what is set on it: apply() sets what a call needs and the handle does not hold, and clears what it holds and
    the call does not want - nothing else, so a session's calls change exactly what differs"""

    def __init__(self, vlq=(3, 2)):
        self.enc = M.Mpeg2Encoder(6, 6, *vlq)
        self.vlq = vlq
        self.held = dict(NOTHING)

    def close(self):
        self.enc.close()

    def apply(self, c):
        assert c["vlq"] == self.vlq
        e, want, held = self.enc, resolved(c), self.held
        if want["size"] != held["size"]:
            e.set_frame_size(*(want["size"] or (0, 0, "module")))
        for key, option in (("conformant", "conformant"), ("stats", "stats"), ("chunk", "batch_frames"), ("split", "split_streams"),
                            ("cap", "gop_bytes_max"), ("cut", "scene_cut")):
            if want[key] != held[key]:
                e.set_option(option, want[key])
        if want["levels"] != held["levels"]:
            e.set_gop_levels(want["levels"])
        if want["starts"] != held["starts"]:
            e.set_gop_starts(want["starts"])
        if want["desc"] != held["desc"]:
            e.set_stream_desc(D.struct(dict(want["desc"])) if want["desc"] else None)
        if want["seqs"] != held["seqs"]:
            e.set_sequences(want["seqs"])
        if held["recon"] and not want["recon"]:              # (prepare() sets the buffers a call wants: they are new for every call)
            e.set_recon_out(None, 0)
        if held["mux"] and not want["mux"]:
            e.set_mux_out(None)
        self.held = want

    def prepare(self, c):
        """everything set and the buffers filled -> what start() needs"""
        import torch
        e = self.enc
        self.apply(c)
        x = C.source(c)
        n = len(x)
        w, h, header = c["geom"]
        xs, ys = M.fit_size(w, h)
        k = dict(c=c, d_in=dev(x), d_out=filled(C.stream_room(c), C.SENTINEL), d_recon=None, d_mux=None, nb=None)
        if c["recon"]:
            nbytes = n * M.frame_bytes(w, h, c["recon"])
            k["d_recon"] = filled(nbytes + C.GUARD, C.FILL)
            e.set_recon_out(k["d_recon"].data_ptr(), nbytes, c["recon"])
        if c["mux"]:
            k["d_mux"] = filled(C.mux_room(c), C.SENTINEL)
            e.set_mux_out(c["mux"], k["d_mux"].data_ptr(), k["d_mux"].numel())
        torch.cuda.synchronize()
        k["args"] = (k["d_in"].data_ptr(), n, k["d_out"].data_ptr(), k["d_out"].numel(), xs, ys, c["pf"])
        return k

    def start(self, k):
        """the call started (and, blocking, finished) -> what finish() needs"""
        e, c, a = self.enc, k["c"], k["args"]
        begin = c["entry"] == "begin"
        if c["kind"] == "444":
            r = (e.encode_resident_begin if begin else e.encode_resident)(*a)
        elif c["kind"] in ("i420", "nv12"):
            r = (e.encode_resident420_begin if begin else e.encode_resident420)(*a, c["kind"])
        else:
            r = (e.encode_resident_rgb_begin if begin else e.encode_resident_rgb)(*a, c["kind"], C.matrix_of(c))
        k["nb"] = None if begin else r
        return k

    def begin(self, c):
        return self.start(self.prepare(c))

    def finish(self, k):
        """-> everything the call handed back, as compose_cases.render lays it out"""
        e = self.enc
        nb = e.encode_resident_end() if k["nb"] is None else k["nb"]
        got = dict(stream_buf=k["d_out"].cpu().numpy(), nbytes=nb,
                   recon_buf=k["d_recon"].cpu().numpy() if k["d_recon"] is not None else None,
                   mux_buf=k["d_mux"].cpu().numpy() if k["d_mux"] is not None else None)
        got.update(self.reports())
        return got

    def reports(self):
        e = self.enc
        got = dict(sequence_report=e.sequence_report(), gop_report=e.gop_report(), scene_report=e.scene_report(),
                   picture_stats=e.picture_stats(), mux_report=e.mux_report())
        assert not any(len(v) for v in (e.sequence_report(), e.gop_report(), e.scene_report(), e.picture_stats(), e.mux_report())), "popped"
        return got

    def run(self, c, what=""):
        C.check(self.finish(self.begin(c)), C.expected(c), what or C.name_of(c))

    def port(self, c, what=""):
        """the same through push_frames / encode()"""
        assert c["entry"] == "port"
        self.apply(c)
        xs, ys = M.fit_size(*c["geom"][:2])
        x = C.source(c)
        if c["kind"] == "444":
            s = self.enc.encode(x, xs, ys, c["pf"])
        else:
            s = self.enc.encode(x, xs, ys, c["pf"], layout=c["kind"], matrix=C.matrix_of(c))
        got = dict(stream_buf=np.frombuffer(s, np.uint8), nbytes=len(s), recon_buf=None, mux_buf=None)
        got.update(self.reports())
        C.check(got, C.expected(c), what or C.name_of(c, C.PORT_FACTORS))


def one(c, what=""):
    h = Handle(c["vlq"])
    try:
        h.run(c, what)
    finally:
        h.close()


# ---- every pair ----
@pytest.mark.parametrize("c", C.pairs(), ids=[C.name_of(c) for c in C.pairs()])
def test_every_pair(c):
    one(c)


@pytest.mark.parametrize("entry", ["block", "begin"])
@pytest.mark.parametrize("name", sorted(C.maximal()))
def test_every_maximal_set(name, entry):
    one(dict(C.maximal()[name], entry=entry), name)


# ---- sessions ----
@pytest.mark.parametrize("seed,vlq", C.SESSIONS)
def test_session_on_one_handle(seed, vlq):
    """a dozen calls that change several settings and the geometry at once; afterwards everything is cleared and a plain call is the
    oracle's plain stream with all five report queues empty"""
    calls = C.session(seed, vlq)
    h = Handle(vlq)
    try:
        for k, c in enumerate(calls):
            h.run(c, "call %d %s" % (k, C.name_of(c)))
        plain = C.call(vlq=vlq)
        k = h.begin(plain)
        assert h.held == NOTHING
        got = h.finish(k)
        want = G.encoded(C.planes(plain), 96, 64, 2, vlq[1], VL=vlq[0])[0]
        assert got["nbytes"] == len(want) and got["stream_buf"][:len(want)].tobytes() == want
        assert (got["stream_buf"][len(want):] == C.SENTINEL).all()
        assert not any(len(got[name]) for name in C.REPORTS)
    finally:
        h.close()


def test_strips_and_port_after_a_call_that_sampled_everything():
    """one handle: after each maximal set's resident call everything is cleared, and the plain frames through the strip entries and
    then through the port are the oracle's plain stream with all five report queues empty - no entry sees what another's sampled"""
    import torch
    plain = C.call()
    frames = C.planes(plain)
    want = G.encoded(frames, 96, 64, 2, 2, VL=3)[0]
    d_clip = dev(frames)
    h = Handle()
    try:
        for name, c in sorted(C.maximal().items()):
            h.run(c, name)
            h.apply(plain)
            assert h.held == NOTHING
            engine = M.parallel.GpuStripEngine(h.enc, d_clip, 6, 4, plain["pf"], "cuda:0")
            out = M.parallel.encode_strips(engine, 0, 1)
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == want, "strips after " + name
            assert not any(len(v) for v in h.reports().values())
            assert h.enc.encode(C.source(plain), 6, 4, plain["pf"]) == want, "the port after " + name
            assert not any(len(v) for v in h.reports().values())
    finally:
        h.close()


def test_two_handles_taking_turns():
    """_begin a, _begin b, _end a, _end b: different rows, different geometry, different buffers"""
    rows = C.session()
    a, b = Handle(C.SESSION_VLQ), Handle(C.SESSION_VLQ)
    try:
        for turn in range(4):
            ca, cb = dict(rows[turn], entry="begin"), dict(rows[(turn + 6) % len(rows)], entry="begin")
            assert ca["geom"][:2] != cb["geom"][:2]
            ka = a.begin(ca)
            kb = b.begin(cb)
            C.check(a.finish(ka), C.expected(ca), "a, turn %d %s" % (turn, C.name_of(ca)))
            C.check(b.finish(kb), C.expected(cb), "b, turn %d %s" % (turn, C.name_of(cb)))
    finally:
        a.close()
        b.close()


# ---- refused pairs ----
def refused(h, c, fn):
    """the call is refused with M2V_E_STATE, m2v_last_error names the function, no output buffer changes"""
    import torch
    k = h.prepare(c)
    with pytest.raises(M.M2VError) as err:
        h.start(k)
    assert "(%d)" % E_STATE in str(err.value) and fn in str(err.value), str(err.value)
    assert fn.encode() in h.enc._L.m2v_last_error(h.enc._h)
    torch.cuda.synchronize()
    for name, value in (("d_out", C.SENTINEL), ("d_recon", C.FILL), ("d_mux", C.SENTINEL)):
        assert (k[name].cpu().numpy() == value).all(), "a refused call wrote into " + name
    assert not any(len(v) for v in h.reports().values())


@pytest.mark.parametrize("pair", C.EXCLUDED, ids=["%s_%s-%s_%s" % (a + b) for a, b in C.EXCLUDED])
@pytest.mark.parametrize("kind", ["444", "nv12", "rgb24"])
def test_refused_pairs(pair, kind):
    (fa, la), (fb, lb) = pair
    c = C.call(kind=kind, recon="i420", mux="ts", stats=1, chunk=4, **{fa: la, fb: lb})
    assert not C.legal(c)
    h = Handle()
    try:
        refused(h, c, {"444": "m2v_encode_resident:", "nv12": "m2v_encode_resident420:", "rgb24": "m2v_encode_resident_rgb:"}[kind])
        # the next legal call on the same handle is right: either half of the pair alone
        h.run(dict(c, **{fb: C.OFF[fb]}), "first half alone")
        h.run(dict(c, **{fa: C.OFF[fa]}), "second half alone")
    finally:
        h.close()


@pytest.mark.parametrize("setting", C.PORT_EXCLUDED, ids=["%s_%s" % s for s in C.PORT_EXCLUDED])
@pytest.mark.parametrize("kind", ["444", "nv12", "rgb24"])
def test_port_refusals(setting, kind):
    f, v = setting
    c = C.call(kind=kind, **{f: v})
    assert C.legal(c) and not C.legal(dict(c, entry="port"))
    h = Handle()
    try:
        h.apply(c)
        d_recon, d_mux = filled(1 << 20, C.FILL), filled(1 << 20, C.SENTINEL)
        if c["recon"]:
            h.enc.set_recon_out(d_recon.data_ptr(), d_recon.numel(), c["recon"])
        if c["mux"]:
            h.enc.set_mux_out(c["mux"], d_mux.data_ptr(), d_mux.numel())
        x = C.source(c)
        with pytest.raises(M.M2VError) as err:
            if kind == "444":
                h.enc.push_frames(6, 4, c["pf"], x)
            elif kind == "nv12":
                h.enc.push_frames420(6, 4, c["pf"], x, kind)
            else:
                h.enc.push_rgb(6, 4, c["pf"], x, kind)
        fn = {"444": "m2v_push_frames:", "nv12": "m2v_push_frames420:", "rgb24": "m2v_push_rgb:"}[kind]
        assert "(%d)" % E_STATE in str(err.value) and fn.encode() in h.enc._L.m2v_last_error(h.enc._h), str(err.value)
        assert (d_recon.cpu().numpy() == C.FILL).all() and (d_mux.cpu().numpy() == C.SENTINEL).all()
        assert not h.enc.busy
        h.enc.set_recon_out(None, 0)
        h.enc.set_mux_out(None)
        h.port(C.call(entry="port", kind=kind, desc="repeat", stats=1, rate="sched", chunk=4), "the next legal call")
    finally:
        h.close()


# ---- the port path ----
@pytest.mark.parametrize("c", C.port_pairs(), ids=[C.name_of(c, C.PORT_FACTORS) for c in C.port_pairs()])
def test_port_path(c):
    h = Handle(c["vlq"])
    try:
        h.port(c)
    finally:
        h.close()


def test_port_session_on_one_handle():
    """the port path's rows of one (VECTOR_LEVEL, Q_LEVEL) one after the other on one handle, then a resident call, then the port again"""
    rows = [c for c in C.port_pairs() if c["vlq"] == C.SESSION_VLQ]
    h = Handle(C.SESSION_VLQ)
    try:
        for c in rows[:4]:
            h.port(c)
        h.run(C.maximal()["cap"])
        h.port(rows[-1])
    finally:
        h.close()


# ---- encode_tensor / encode_batch ----
def test_encode_tensor_and_encode_batch_with_a_maximal_set():
    import torch
    h = Handle()
    e = h.enc
    try:
        plain = C.call(kind="rgb24")
        t_plain = dev(C.source(plain)).reshape(C.N, 64, 96, 3)
        want_plain = G.encoded(C.planes(plain), 96, 64, 2, 2)[0]
        # the list, the detector and a schedule, everything else on
        c = dict(C.maximal()["list_detector_schedule"], kind="rgb24", conformant=0, chunk=96, split=2)
        w, hh, header = c["geom"]
        want = C.expected(c)
        t = dev(C.source(c)).reshape(C.N, hh, w, 3)
        got, records, rec = e.encode_tensor(t, c["pf"], matrix=C.matrix_of(c), header=header, stats=True, gop_levels=C.levels_of(c),
                                            gop_starts=C.starts_of(c), scene_cut=C.cut_of(c), recon=c["recon"],
                                            desc=D.struct(C.desc_of(c)), container=c["mux"])
        assert got.cpu().numpy().tobytes() == want["containers"][0]
        assert np.array_equal(rec.cpu().numpy(), want["recon"])
        r = h.reports()
        r["picture_stats"] = records
        r["mux_report"] = want["mux_report"]                                   # (encode_tensor has popped it: the container says it)
        shaped = C.render(c, want)
        shaped.update(r)
        C.check(shaped, want, "encode_tensor: the reports")
        assert e.encode_tensor(t_plain, 2).cpu().numpy().tobytes() == want_plain      # the handle's own settings are back
        assert not any(len(v) for v in h.reports().values())
        # a batch with a schedule, everything else on
        c = dict(C.maximal()["sequences_schedule"], kind="rgb24", conformant=0, chunk=96, split=2)
        want = C.expected(c)
        got, where, records, rec = e.encode_batch(t, c["pf"], lengths=C.lengths_of(c), matrix=C.matrix_of(c), header=c["geom"][2], stats=True,
                                                  gop_levels=C.levels_of(c), recon=c["recon"], desc=D.struct(C.desc_of(c)), container=c["mux"])
        g = got.cpu().numpy().tobytes()
        lay = X.layout([len(v) for v in want["containers"]], 1 << 40)
        assert where == [(o, nb) for o, nb, _ in lay]
        for b, (o, nb) in enumerate(where):
            assert g[o:o + nb] == want["containers"][b], b
        assert np.array_equal(rec.cpu().numpy(), want["recon"])
        r = h.reports()
        r["picture_stats"] = records
        r["mux_report"] = want["mux_report"]
        shaped = C.render(c, want)
        shaped.update(r)
        C.check(shaped, want, "encode_batch: the reports")
        stream, offsets = e.encode_batch(t, c["pf"], lengths=C.lengths_of(c), header=c["geom"][2], gop_levels=C.levels_of(c),
                                         desc=D.struct(C.desc_of(c)))
        assert stream.cpu().numpy().tobytes() == want["stream"] and offsets == want["offsets"]
        assert e.encode_tensor(t_plain, 2).cpu().numpy().tobytes() == want_plain
        assert not any(len(v) for v in h.reports().values())
        torch.cuda.synchronize()
    finally:
        h.close()
