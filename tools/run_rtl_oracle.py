#!/usr/bin/env python3
"""Cross-check against the REAL RTL wherever a Verilog simulator exists.

    python tools/run_rtl_oracle.py [--rtl /path/to/mpeg2encoder.v] [--keep]

For a few small seeded clips and parameter sets it (1) writes the clip as planar yuv444p, (2) writes a
self-contained Verilog-2001 testbench (generated here, parameterised, same stimulus protocol as
SIM/tb_mpeg2encoder.v: one beat per clock, stop pulse with i_en=0, o_data byte 0 first), (3) runs
`iverilog -g2001` + `vvp -n` (SIM/tb_run_iverilog.bat:2-3) - or, where only Verilator (>= 5) is installed, `verilator --binary
--timing` -, (4) compares the .m2v byte for byte with the CPU oracle and reports clocks/s, and (5) where a GPU and the built product
are at hand, drives the product's own testbench counterpart (m2v_tb, the same files through the C-ABI) and prints ONE three-way verdict
line:  RTL == oracle == product.  The generated testbench also writes one line per macroblock at the moment the RTL's stage T latches it
(frame, row, column, inter flag, vector, coded flags - hierarchical references to g_inter, g_mvx, g_mvy, s_nzflags at s_en_blk,
RTL:2630-2637), which is compared with the oracle's dump: on first contact a mismatch is localised to a STAGE, not to a byte offset.  The two hand-derived 160-byte known-answer streams (tests/golden/) go first: a
simulator whose `$fwrite("%c")` drops the 0x00 bytes of the start codes fails there, before anything is concluded
from the seeded clips.  Without a simulator or without the RTL file it prints "RTL oracle unavailable" and exits 0 (this is the case in
the build image and on the GPU box).  The last stdout line is a JSON object (bench.py copies it into its `rtl_sim` entry).
"""
import argparse
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TB = r"""
`timescale 1ps/1ps
module tb;
localparam XL = %(XL)d, YL = %(YL)d, W = %(W)d, H = %(H)d, NF = %(NF)d, NBEATS = %(NBEATS)d;
reg rstn = 1'b1, clk = 1'b0;
always #10000 clk = ~clk;
reg i_en = 0, i_stop = 0;
reg [XL:0] xs16 = W/16;  reg [YL:0] ys16 = H/16;
reg [7:0] Y0,Y1,Y2,Y3,U0,U1,U2,U3,V0,V1,V2,V3;
wire busy, o_en, o_last;  wire [255:0] o_data;
mpeg2encoder #(.XL(XL), .YL(YL), .VECTOR_LEVEL(%(VL)d), .Q_LEVEL(%(Q)d)) dut (
  .rstn(rstn), .clk(clk), .i_xsize16(xs16), .i_ysize16(ys16), .i_pframes_count(8'd%(PF)d),
  .i_en(i_en), .i_Y0(Y0), .i_Y1(Y1), .i_Y2(Y2), .i_Y3(Y3), .i_U0(U0), .i_U1(U1), .i_U2(U2), .i_U3(U3),
  .i_V0(V0), .i_V1(V1), .i_V2(V2), .i_V3(V3), .i_sequence_stop(i_stop), .o_sequence_busy(busy),
  .o_en(o_en), .o_last(o_last), .o_data(o_data));
reg [7:0] mem [0:NF*W*H*3-1];
integer fi, fo, k, f, p, b, clocks;
initial begin
  fi = $fopen("%(IN)s", "rb");  fo = $fopen("%(OUT)s", "wb");
  for (k = 0; k < NF*W*H*3; k = k + 1) mem[k] = $fgetc(fi);
  $fclose(fi);
  repeat(4) @(posedge clk); rstn <= 1'b0; repeat(4) @(posedge clk); rstn <= 1'b1; @(posedge clk);
  fork
    begin
      for (b = 0; b < NBEATS; b = b + 1) begin
        f = b / (W*H/4);  p = (b %% (W*H/4)) * 4;
        i_en <= 1'b1;
        Y0 <= mem[f*W*H*3 + p];           Y1 <= mem[f*W*H*3 + p + 1];           Y2 <= mem[f*W*H*3 + p + 2];           Y3 <= mem[f*W*H*3 + p + 3];
        U0 <= mem[f*W*H*3 + W*H + p];     U1 <= mem[f*W*H*3 + W*H + p + 1];     U2 <= mem[f*W*H*3 + W*H + p + 2];     U3 <= mem[f*W*H*3 + W*H + p + 3];
        V0 <= mem[f*W*H*3 + 2*W*H + p];   V1 <= mem[f*W*H*3 + 2*W*H + p + 1];   V2 <= mem[f*W*H*3 + 2*W*H + p + 2];   V3 <= mem[f*W*H*3 + 2*W*H + p + 3];
        @(posedge clk);
        i_en <= 1'b0;
      end
      i_stop <= 1'b1; @(posedge clk); i_stop <= 1'b0; @(posedge clk);
    end
    begin
      clocks = 0;
      while (~busy) @(posedge clk);
      while (busy) begin
        if (o_en) for (k = 0; k < 32; k = k + 1) $fwrite(fo, "%%c", o_data[k*8 +: 8]);
        clocks = clocks + 1;
        @(posedge clk);
      end
    end
  join
  $fclose(fo);
  $fclose(fd);
  $display("CLOCKS %%0d", clocks);
  $finish;
end
// One line per macroblock at the moment stage T latches it (RTL:2630-2637: s_en_blk in PUT_IDLE): frame, row, column, inter flag, the
// transmitted vector, the six coded flags - so that a first mismatch is localised to a STAGE (decision / vector / coded pattern), not to a byte
// offset.  Hierarchical references into the module under test (Verilator: --public-flat-rw).
integer fd, mbf;
initial begin fd = $fopen("%(DUMP)s", "w"); mbf = -1; end
always @(posedge clk) if (dut.s_en_blk) begin
  if (dut.g_y16 == 0 && dut.g_x16 == 0) mbf = mbf + 1;
  $fdisplay(fd, "MB %%0d %%0d %%0d %%0d %%0d %%0d %%0d", mbf, dut.g_y16, dut.g_x16, dut.g_inter, $signed(dut.g_mvx), $signed(dut.g_mvy), dut.s_nzflags);
end
endmodule
"""

CASES = [
    # W, H, frames, pframes, XL, YL, VL, Q, stop_beats (None = all)
    (64, 64, 1, 0, 4, 4, 1, 2, None),
    (64, 64, 3, 2, 4, 4, 3, 2, None),
    (96, 64, 5, 4, 5, 4, 3, 2, None),
    (128, 96, 4, 3, 6, 6, 2, 3, None),
    (96, 80, 4, 1, 6, 6, 1, 1, 3 * (96 * 80 // 4) + 77),
    (128, 128, 9, 8, 7, 7, 3, 4, None),
]


def find_simulator():
    """-> (name, build(tb, rtl, workdir, tag) -> argv of the simulation) or (None, None).  iverilog is the reference's own flow
    (SIM/tb_run_iverilog.bat:2-3); Verilator 5 can run the same generated testbench (`--binary --timing`: delays, @(posedge), fork / join)."""
    iv, vvp, ver = shutil.which("iverilog"), shutil.which("vvp"), shutil.which("verilator")
    if iv and vvp:
        def build(tb, rtl, work, tag):
            sim = os.path.join(work, tag + ".out")
            subprocess.check_call([iv, "-g2001", "-o", sim, tb, rtl])
            return [vvp, "-n", sim]
        return "iverilog", build
    if ver:
        def build(tb, rtl, work, tag):
            obj = os.path.join(work, "obj_" + tag)
            subprocess.check_call([ver, "--binary", "--timing", "--public-flat-rw", "-Wno-fatal", "-Wno-lint", "-Wno-style", "--top-module", "tb", "--Mdir", obj,
                                   "-o", "sim", tb, rtl], stdout=subprocess.DEVNULL)
            return [os.path.join(obj, "sim")]
        return "verilator", build
    return None, None


def product_bytes(clip_path, W, H, pf, XL, YL, VL, Q, nframes, work, tag):
    """the product's testbench counterpart (m2v_tb: file -> C-ABI beats -> file) on the same clip; None without a GPU or without the
    built binary.  m2v_tb pushes the complete frames of the file (TB:220), so it serves the cases that stop on a frame boundary."""
    tb = os.path.join(ROOT, "fpga-mpeg2-encoder_amd", "m2v_tb")
    if not os.path.exists(tb) or not product_possible():
        return None                                   # "not run": no binary, or no GPU on this host
    out = os.path.join(work, tag + ".product.m2v")
    r = subprocess.run([tb, "-XL", str(XL), "-YL", str(YL), "-VL", str(VL), "-Q", str(Q), "-p", str(pf), clip_path, str(W), str(H), out],
                       capture_output=True, text=True)
    if r.returncode != 0 or not os.path.exists(out):
        # the product RAN and failed: that is a mismatch, not an absence
        sys.stderr.write("m2v_tb failed on %s (exit code %d):\n%s\n" % (tag, r.returncode, (r.stderr or r.stdout)[-2000:]))
        return PRODUCT_FAILED
    return open(out, "rb").read()


PRODUCT_FAILED = b"\xffm2v_tb failed"             # never equal to a stream (a stream starts with 00 00 01 B3)


def product_possible():
    """is there a GPU for m2v_tb to run on?  (KFD topology: a node with SIMDs; no HIP call from this process)"""
    import glob
    for f in glob.glob("/sys/class/kfd/kfd/topology/nodes/*/properties"):
        try:
            for ln in open(f):
                k, _, val = ln.partition(" ")
                if k == "simd_count" and int(val) > 0:
                    return True
        except (OSError, ValueError):
            pass
    return False


def compare_mb_dump(path, dump, W, H, limit=5):
    """The RTL's per-macroblock lines (the generated testbench's $fdisplay at s_en_blk) against the oracle's dump of the same
    sequence: -> (macroblocks compared, [first mismatches as text]).  A macroblock's vector is compared only when it is inter
    (the RTL's g_mvx / g_mvy hold the search result for intra macroblocks too; nothing of it is transmitted)."""
    mbw = W // 16
    bad, n = [], 0
    if not os.path.exists(path):
        return 0, ["no per-macroblock dump was written (simulator without hierarchical references?)"]
    for ln in open(path):
        t = ln.split()
        if len(t) != 8 or t[0] != "MB":
            continue
        f, y, x, inter, mvx, mvy, nz = (int(v) for v in t[1:])
        if f < 0 or f >= dump["mb_inter"].shape[0] or y * mbw + x >= dump["mb_inter"].shape[1]:
            bad.append("macroblock (frame %d, row %d, column %d) outside the oracle's sequence" % (f, y, x))
            continue
        i = y * mbw + x
        n += 1
        o_inter, o_cbp = int(dump["mb_inter"][f, i]), int(dump["mb_cbp"][f, i])
        o_mv = (int(dump["mb_mvx"][f, i]), int(dump["mb_mvy"][f, i]))
        what = []
        if inter != o_inter:
            what.append("intra/inter decision (stage F, RTL:1790-1816): RTL %d, oracle %d" % (inter, o_inter))
        elif inter and (mvx, mvy) != o_mv:
            what.append("motion vector (stage F, RTL:1634-1829): RTL (%d, %d), oracle (%d, %d)" % (mvx, mvy, o_mv[0], o_mv[1]))
        if nz != o_cbp:
            what.append("coded flags (stages G-S, RTL:1972-2468): RTL %s, oracle %s" % (format(nz, "06b"), format(o_cbp, "06b")))
        if what and len(bad) < limit:
            bad.append("frame %d, macroblock row %d column %d: %s" % (f, y, x, "; ".join(what)))
        elif what:
            bad.append(None)
    return n, bad


def main():
    import json
    ap = argparse.ArgumentParser()
    ap.add_argument("--rtl", default=os.environ.get("M2V_RTL", ""), help="the reference's RTL/mpeg2encoder.v (default: $M2V_RTL)")
    ap.add_argument("--keep", action="store_true")
    args = ap.parse_args()
    simname, build = find_simulator()
    if not simname or not os.path.exists(args.rtl):
        print("RTL oracle unavailable (simulator=%s rtl=%s): parity stays pinned by the oracle's own tests" % (simname, os.path.exists(args.rtl)))
        print(json.dumps({"available": False, "simulator": simname, "rtl": os.path.exists(args.rtl)}))
        return 0
    import m2v_load
    from oracle import m2v_oracle_ctypes as orc
    M = m2v_load.load()
    tmp = tempfile.mkdtemp(prefix="m2v_rtl_")

    def simulate(clip, W, H, nf, pf, XL, YL, VL, Q, nbeats, tag):
        fin, fout, ftb = (os.path.join(tmp, "%s.%s" % (tag, e)) for e in ("yuv", "m2v", "v"))
        clip.tofile(fin)
        open(ftb, "w").write(TB % dict(XL=XL, YL=YL, W=W, H=H, NF=nf, NBEATS=nbeats, VL=VL, Q=Q, PF=pf, IN=fin, OUT=fout, DUMP=os.path.join(tmp, tag + ".mb")))
        argv = build(ftb, args.rtl, tmp, tag)
        t0 = time.time()
        log = subprocess.run(argv, capture_output=True, text=True).stdout
        dt = time.time() - t0
        clocks = [int(l.split()[1]) for l in log.splitlines() if l.startswith("CLOCKS")]
        return open(fout, "rb").read(), dt, (clocks[0] if clocks else None), fin

    # 1. the hand-derived known-answer streams: does this simulator write every byte, NULs included?
    kat_ok = True
    for kind in ("gray", "black"):
        f = M.synth.degenerate(kind, 64, 64, 1)
        got, _, _, _ = simulate(f, 64, 64, 1, 0, 4, 4, 1, 2, 64 * 64 // 4, "kat_" + kind)
        want = open(os.path.join(ROOT, "tests", "golden", "kat_%s_64x64.m2v" % kind), "rb").read()
        same = got == want
        kat_ok &= same
        print("known answer %-5s 64x64: RTL under %s %d bytes -> %s%s" % (kind, simname, len(got), "IDENTICAL" if same else "DIFFERENT",
              "" if same else "  (if only the 0x00 bytes are missing: this simulator drops NUL on %c - SURVEY.md 8(c))"))
    # 2. seeded clips, three ways
    bad_oracle = bad_product = product_cases = mb_total = mb_wrong = 0
    px = secs = 0.0
    for ci, (W, H, nf, pf, XL, YL, VL, Q, stop) in enumerate(CASES):
        clip = M.synth.clip(W, H, nf, clip_index=100 + ci, scene_len=3)
        nbeats = nf * W * H // 4 if stop is None else stop
        got, dt, clocks, fin = simulate(clip, W, H, nf, pf, XL, YL, VL, Q, nbeats, "c%d" % ci)
        want, dump = orc.encode(clip, W // 16, H // 16, pf, XL, YL, VL, Q, nbeats=nbeats, dump=True)
        prod = product_bytes(fin, W, H, pf, XL, YL, VL, Q, nf, tmp, "c%d" % ci) if stop is None else None
        ok = got == want
        bad_oracle += not ok
        mb_n, mb_bad = compare_mb_dump(os.path.join(tmp, "c%d.mb" % ci), dump, W, H)
        mb_total += mb_n
        mb_wrong += len(mb_bad)
        for line in [b for b in mb_bad if b][:5]:
            print("    first differences by stage: " + line)
        if prod is not None:
            product_cases += 1
            bad_product += prod != got
        px += nbeats * 4
        secs += dt
        print("case %d %dx%d x%d pf=%d VL=%d Q=%d: RTL %d bytes, oracle %d bytes -> %s; product (m2v_tb) %s   (%.1f s, %s clocks, %.4f MPixels/s)"
              % (ci, W, H, nf, pf, VL, Q, len(got), len(want), "IDENTICAL" if ok else "DIFFERENT",
                 "not run" if prod is None else "FAILED" if prod == PRODUCT_FAILED else "IDENTICAL to the RTL" if prod == got else "DIFFERENT from the RTL", dt,
                 clocks if clocks is not None else "?", nbeats * 4 / dt * 1e-6))
    verdict = {"available": True, "simulator": simname, "known_answers_identical": kat_ok, "cases": len(CASES),
               "rtl_equals_oracle": bad_oracle == 0 and kat_ok, "product_cases": product_cases,
               "rtl_equals_product": (bad_product == 0) if product_cases else None,
               "macroblocks_compared_by_stage": mb_total, "macroblocks_differing_by_stage": mb_wrong,
               "rtl_sim_MPixels_per_s": round(px / secs * 1e-6, 5) if secs > 0 else None, "cores": 1}
    print("three-way verdict: RTL %s oracle; RTL %s product (%d of %d cases through m2v_tb); simulator %s"
          % ("==" if verdict["rtl_equals_oracle"] else "!=", "==" if verdict["rtl_equals_product"] else ("!=" if product_cases else "?="),
             product_cases, len(CASES), simname))
    print(json.dumps(verdict))
    if not args.keep:
        shutil.rmtree(tmp, ignore_errors=True)
    # exit code: bit 0 = the RTL and the ORACLE differ (or a known answer does), bit 1 = the RTL and the PRODUCT differ (or m2v_tb failed)
    return (1 if (bad_oracle or not kat_ok) else 0) | (2 if bad_product else 0)


if __name__ == "__main__":
    sys.exit(main())
