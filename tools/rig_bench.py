#!/usr/bin/env python3
"""One rig call against what a caller had before it, interleaved in ONE process on ONE device (tools/ab.py's method:
the arms take turns round by round; devices and runs differ by ~10 %, so nothing else ranks them).  GPU box only.

  A  d2pc_rig_process_device: n cameras, n Qs, one merged cloud
  B  n x (d2pc_set_q + d2pc_process_device of one frame) on one context and stream: n separate clouds
  C  d2pc_process_device on the same batch with ONE Q (what the batch entry point offers: the price of the table in
     PARITY, the price of recomputing in the scatter in COMPACT)

  python tools/rig_bench.py            ->  profiles/rig_bench.txt
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import disparity_to_point_cloud_amd as d2pc  # noqa: E402

CASES = [(4, 752, 480, "u8", 40), (8, 752, 480, "u8", 40), (16, 752, 480, "u8", 40), (6, 1920, 1080, "f32", 40),
         (16, 3840, 2160, "f32", 40)]
DT = {"f32": (d2pc.DTYPE_F32, torch.float32, 1.0), "u8": (d2pc.DTYPE_U8, torch.uint8, 0.125)}


def qs_for(n, posed):
    out = []
    for f in range(n):
        q = d2pc.make_q(fx=714.24 - 3.0 * f, fy=713.5 - 3.0 * f, cx=376.0 + f, cy=240.0 - f)
        if posed:
            a = 2.0 * math.pi * f / n + 0.1
            t = np.array([[math.cos(a), 0, math.sin(a), 0.1 * f], [0, 1, 0, 0.02], [-math.sin(a), 0, math.cos(a), 0.05], [0, 0, 0, 1.0]])
            q = d2pc.rig_compose_q(t, q).reshape(16)
        out.append(q)
    return out


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters   # us per call


def fmt(v):
    return "%8.1f (%7.1f .. %7.1f)" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--holes", type=float, default=0.3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_bench.txt"))
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    lines = ["# tools/rig_bench.py --rounds %d --iters %d --holes %.2f" % (a.rounds, a.iters, a.holes),
             "# device draw: %s, %d CUs, %.0f GiB (one device, one process; arms interleaved round by round)" % (
                 prop.name, prop.multi_processor_count, prop.total_memory / 2**30),
             "# A = one d2pc_rig_process_device; B = n x (d2pc_set_q + d2pc_process_device of one frame); C = d2pc_process_device, batch, one Q",
             "# us per call: median (min .. max) over the rounds; B spread = B max / B min in this run",
             "%-26s %-8s %-7s %-30s %-30s %-30s %6s %9s %6s" % ("case", "mode", "Qs", "A", "B", "C", "B/A", "B spread", "A/C")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    for n, w, h, dt, border in CASES:
        code, tdt, scale = DT[dt]
        if dt == "f32":
            frames = torch.rand((n, h, w), generator=gen, device="cuda") * 127.5 + 0.5
        else:
            frames = torch.randint(8, 256, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
        frames[torch.rand((n, h, w), generator=gen, device="cuda") < a.holes] = 0
        roi_n = d2pc.roi_points(w, h, border)
        pts = torch.empty((n * roi_n, 4), dtype=torch.float32, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        es = frames.element_size()
        for mode, mname in ((d2pc.MODE_PARITY, "PARITY"), (d2pc.MODE_COMPACT, "COMPACT")):
            for posed in (False, True):
                qs = qs_for(n, posed)
                with d2pc.Context(q=qs[0], border=border, mode=mode) as ctx, d2pc.RigSession(ctx, n, w, h, code, qs) as rig:
                    def arm_a():
                        rig.process_device(frames.data_ptr(), scale, w * es, h * w * es, pts.data_ptr(), None, n * roi_n,
                                           counts.data_ptr(), offsets.data_ptr(), s)

                    def arm_b():
                        for f in range(n):
                            ctx.set_q(qs[f])
                            ctx.process_device(frames.data_ptr() + f * h * w * es, code, scale, w, h, w * es, h * w * es, 1,
                                               pts.data_ptr() + f * roi_n * 16, None, roi_n, counts.data_ptr() + 4 * f, s)

                    def arm_c():
                        ctx.set_q(qs[0])
                        ctx.process_device(frames.data_ptr(), code, scale, w, h, w * es, h * w * es, n, pts.data_ptr(), None,
                                           roi_n, counts.data_ptr(), s)

                    arms = (arm_a, arm_b, arm_c)
                    for fn in arms:   # warm-up: allocations, code objects
                        fn()
                    torch.cuda.synchronize()
                    t = [[], [], []]
                    for r in range(a.rounds):
                        for k in range(3):
                            k2 = (k + r) % 3   # the order rotates too
                            t[k2].append(timed(arms[k2], a.iters))
                    ctx.check_async_error()
                ma, mb, mc = (float(np.median(x)) for x in t)
                lines.append("%-26s %-8s %-7s %-30s %-30s %-30s %6.2f %9.2f %6.2f" % (
                    "%2d x %dx%d %s b%d" % (n, w, h, dt, border), mname, "posed" if posed else "stereo", fmt(t[0]), fmt(t[1]), fmt(t[2]),
                    mb / ma, max(t[1]) / min(t[1]), ma / mc))
                print(lines[-1], flush=True)
        del frames, pts
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
