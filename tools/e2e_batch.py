"""tools/e2e_batch.py — many short clips, one stream each: one resident call per clip against one call for the batch
(m2v_set_sequences), one JSON line.

Workload A: 64 clips x 9 frames of 320 x 240, pframes_count 8.  Workload B: 16 clips x 30 frames of 640 x 480, I-only.  Legs, in one
process, alternating in rotating order, each timed over `--steps` passes of the whole workload per round:
  loop    one m2v_encode_resident_begin / _end per clip on two handles taking turns, every clip's stream written to the offset the batch
          uses - the best form a library without m2v_set_sequences offers.  This leg needs nothing new: with M2V_LIB pointing at an
          older build of the library the tool runs it alone (--legs loop), so it can be measured against the parent commit.
  batch1  one call for the batch on one handle, "batch_frames" covering it
  batch2  the same on two handles taking turns
The bytes of all legs are asserted identical before anything is timed.  Reported per leg: best, median and spread (max - min) of the
rounds, in ms per pass over the workload, and batch / loop of the medians.

--trace: no timing - a few batch calls of workload A and a few plain 576-frame sequences of the same size, for a run under
rocprofv3 --kernel-trace --stats, where k_seq_scan's time per chunk stands beside k_frame_scan's.

    python tools/e2e_batch.py [--rounds 9] [--steps 32] [--legs loop,batch1,batch2] [--workloads A,B] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"A": dict(W=320, H=240, clips=64, frames=9, pf=8), "B": dict(W=640, H=480, clips=16, frames=30, pf=0)}
XL = YL = 7
VL, Q = 3, 2


class Work:
    def __init__(self, M, torch, w, with_batch):
        self.M, self.torch, self.w = M, torch, w
        self.n = w["clips"] * w["frames"]
        self.xs, self.ys = w["W"] // 16, w["H"] // 16
        self.fb = 3 * w["W"] * w["H"]
        # every clip its own material: a scene cut at every clip's first frame
        self.clip = M.synth.clip_torch(w["W"], w["H"], self.n, clip_index=3, device="cuda:0", scene_len=w["frames"]).contiguous()
        self.cap = self.n * self.fb // 2 + 64 * w["clips"] + 4096
        self.outs = [torch.empty(self.cap, dtype=torch.uint8, device="cuda:0") for _ in range(2)]
        self.pair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)]
        self.bpair = [M.Mpeg2Encoder(XL, YL, VL, Q) for _ in range(2)] if with_batch else []
        for h in self.bpair:
            h.set_option("batch_frames", self.n)
            h.set_sequences([w["frames"]] * w["clips"])
        # the offsets: every clip alone, once (a stream is whole 32-byte words, so the batch's offsets are the running sum)
        self.off = [0]
        for b in range(w["clips"]):
            nb = self.pair[0].encode_resident(self.clip.data_ptr() + b * w["frames"] * self.fb, w["frames"], self.outs[0].data_ptr() + self.off[-1],
                                              self.cap - self.off[-1], self.xs, self.ys, w["pf"])
            assert nb % 32 == 0
            self.off.append(self.off[-1] + nb)
        torch.cuda.synchronize()
        self.want = self.outs[0][:self.off[-1]].cpu().numpy().tobytes()

    def loop(self, steps, out=0):
        """`steps` passes: a call per clip, two handles taking turns, two clips in flight"""
        w, busy = self.w, [False, False]
        base, dst = self.clip.data_ptr(), self.outs[out].data_ptr()
        for _ in range(steps):
            for b in range(w["clips"]):
                h = self.pair[b & 1]
                if busy[b & 1]:
                    h.encode_resident_end()
                h.encode_resident_begin(base + b * w["frames"] * self.fb, w["frames"], dst + self.off[b], self.off[b + 1] - self.off[b], self.xs, self.ys, w["pf"])
                busy[b & 1] = True
        for k in range(2):
            if busy[k]:
                self.pair[k].encode_resident_end()

    def batch(self, steps, handles):
        busy = [False] * handles
        for s in range(steps):
            k = s % handles
            if busy[k]:
                assert self.bpair[k].encode_resident_end() == self.off[-1]
            self.bpair[k].encode_resident_begin(self.clip.data_ptr(), self.n, self.outs[k].data_ptr(), self.cap, self.xs, self.ys, self.w["pf"])
            busy[k] = True
        for k in range(handles):
            if busy[k]:
                assert self.bpair[k].encode_resident_end() == self.off[-1]

    def run(self, leg, steps):
        if leg == "loop":
            self.loop(steps)
        else:
            self.batch(steps, 1 if leg == "batch1" else 2)

    def verify(self, legs):
        torch = self.torch
        for leg in legs:
            for o in self.outs:
                o.zero_()
            self.run(leg, 2)
            torch.cuda.synchronize()
            used = (0,) if leg != "batch2" else (0, 1)
            for k in used:
                assert self.outs[k][:self.off[-1]].cpu().numpy().tobytes() == self.want, "leg %s writes other bytes" % leg
            if leg != "loop":
                rec = self.bpair[0].sequence_report()
                assert [int(v) for v in rec["offset"]] == self.off[:-1] and int(rec["offset"][-1] + rec["bytes"][-1]) == self.off[-1]

    def close(self):
        for h in self.pair + self.bpair:
            h.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--steps", type=int, default=32, help="passes over the workload per timed round")
    ap.add_argument("--legs", default="loop,batch1,batch2")
    ap.add_argument("--workloads", default="A,B")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import m2v_load
    M = m2v_load.load()
    legs = [x for x in args.legs.split(",") if x]
    with_batch = any(x != "loop" for x in legs)
    if args.trace:
        w = WORKLOADS["A"]
        work = Work(M, torch, w, True)
        work.batch(5, 1)
        plain = M.Mpeg2Encoder(XL, YL, VL, Q)
        plain.set_option("batch_frames", work.n)
        for _ in range(5):
            plain.encode_resident(work.clip.data_ptr(), work.n, work.outs[0].data_ptr(), work.cap, work.xs, work.ys, w["pf"])
        torch.cuda.synchronize()
        plain.close()
        work.close()
        print(json.dumps({"tool": "e2e_batch", "trace": True, "frames": work.n, "calls": 5}))
        return
    res = {"tool": "e2e_batch", "library": os.environ.get("M2V_LIB") or "this tree", "rounds": max(args.rounds, 8), "steps": args.steps,
           "host": "python, ctypes", "workloads": {}}
    for name in args.workloads.split(","):
        w = WORKLOADS[name]
        work = Work(M, torch, w, with_batch)
        work.verify(legs)
        for leg in legs:
            work.run(leg, 2)                      # warm-up: plans cached, buffers allocated
        torch.cuda.synchronize()
        times = {leg: [] for leg in legs}
        for r in range(max(args.rounds, 8)):
            for i in range(len(legs)):
                leg = legs[(r + i) % len(legs)]
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                work.run(leg, args.steps)
                times[leg].append((time.perf_counter() - t0) * 1e3 / args.steps)
        out = dict(w, bytes=work.off[-1], legs={})
        for leg in legs:
            t = times[leg]
            out["legs"][leg] = {"best_ms": round(min(t), 4), "median_ms": round(statistics.median(t), 4), "spread_ms": round(max(t) - min(t), 4),
                                "fps_median": round(work.n / statistics.median(t) * 1e3, 1)}
        if "loop" in legs:
            for leg in legs:
                if leg != "loop":
                    out["legs"][leg]["median_over_loop"] = round(out["legs"][leg]["median_ms"] / out["legs"]["loop"]["median_ms"], 4)
        res["workloads"][name] = out
        work.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
