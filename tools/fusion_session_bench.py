#!/usr/bin/env python3
"""The fusing DisparityCb2 of the C session (d2pc_fusion_node_callback_device): ONE launch (single_launch = 1,
d2pc_node.hip) against the three-launch composition (single_launch = 0), in the same process, interleaved round by
round as tools/ab.py does, so that clock drift hits both alike.  GPU only.

Per case: median, min and max over the rounds of the time per callback, called back to back on one stream (eager) and
as a replayed graph of the one callback.  The decision DESIGN.md section 8c records is printed for the reference
geometry: single_launch defaults to 1 only if it beats the composition by more than the composition's own run-to-run
spread (max - min over its rounds) in this interleaved run.

  python tools/fusion_session_bench.py [--out PATH]
  python tools/fusion_session_bench.py --trace-run 1|0   # 10 fusing callbacks and nothing else: the program for
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fusion_session_bench.py --trace-run 1
  python tools/fusion_session_bench.py --kernel-stats DIR  # kernel names and calls of such a run
"""
import argparse
import csv
import glob
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import disparity_to_point_cloud_amd as d2pc  # noqa: E402

# (label, batch, cols, rows, offset_x, offset_y)
CASES = [("reference 1 x 752x480 -7/15", 1, 752, 480, -7, 15), ("16 x 752x480 -7/15", 16, 752, 480, -7, 15),
         ("32 x 1920x1080", 32, 1920, 1080, 0, 0), ("16 x 3840x2160", 16, 3840, 2160, 0, 0)]
TRACE_REPS = 10


def primed(ctx, batch, cols, rows, ox, oy, single):
    s = d2pc.FusionSession(ctx, cols, rows, ox, oy, batch=batch, single_launch=single)
    shape = (rows, cols) if batch == 1 else (batch, rows, cols)
    g = torch.Generator(device="cuda").manual_seed(1)
    fr = {k: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda", generator=g) for k in ("D1", "S1", "S2", "D2")}
    s.disparity_1(fr["D1"]), s.matching_score_1(fr["S1"]), s.matching_score_2(fr["S2"])
    out = s.disparity_2(fr["D2"])
    torch.cuda.synchronize()
    return s, fr["D2"], out


def rounds_interleaved(fns, iters, rounds):
    """us per call of every fn, `rounds` times, the fns taking turns inside each round."""
    for fn in fns:
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            ts[i].append(e0.elapsed_time(e1) / iters * 1e3)
    return [(float(np.median(t)), float(min(t)), float(max(t))) for t in ts]


def graph_of(fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        fn()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def bench(ctx, lines):
    def say(text):
        print(text, flush=True)
        lines.append(text)

    say(f"device: {torch.cuda.get_device_name(0)}")
    say("fusing DisparityCb2, us per callback: median (min .. max) over the rounds; A = one launch, B = three launches")
    for label, batch, cols, rows, ox, oy in CASES:
        a, fa, oa = primed(ctx, batch, cols, rows, ox, oy, 1)
        b, fb, ob = primed(ctx, batch, cols, rows, ox, oy, 0)
        for topic in oa:  # the two compute the same bytes
            assert torch.equal(oa[topic], ob[topic]), (label, topic)
        pitch, fstride = fa.stride(-2), (fa.stride(0) if fa.dim() == 3 else 0)

        def call(s, f):
            # the raw entry point: no tensor views are built in the timed loop
            ptr = f.data_ptr()
            return lambda: s.callback_device(d2pc.NODE_DISPARITY_2, ptr, pitch, fstride, torch.cuda.current_stream().cuda_stream)

        iters, rounds = (200, 15) if batch == 1 else (20, 9)
        ea, eb = rounds_interleaved([call(a, fa), call(b, fb)], iters, rounds)
        ga, gb = graph_of(call(a, fa)), graph_of(call(b, fb))
        ra, rb = rounds_interleaved([ga.replay, gb.replay], iters, rounds)
        for how, (x, y) in (("eager", (ea, eb)), ("graph", (ra, rb))):
            say(f"{label:28s} n {a.n:4d} {how}: A {x[0]:9.2f} ({x[1]:9.2f} .. {x[2]:9.2f})   B {y[0]:9.2f} ({y[1]:9.2f} .. {y[2]:9.2f})"
                f"   B/A {y[0] / x[0]:5.2f}   B's spread {y[2] - y[1]:7.2f}")
        if label.startswith("reference"):
            for how, (x, y) in (("eager", (ea, eb)), ("graph", (ra, rb))):
                gain, spread = y[0] - x[0], y[2] - y[1]
                say(f"  decision ({how}): the single launch gains {gain:.2f} us, the composition's spread is {spread:.2f} us"
                    f" -> single_launch default {'1' if gain > spread else '0'}")
        del ga, gb
        a.close(), b.close()


def trace_run(ctx, single):
    s, f, _ = primed(ctx, 1, 752, 480, -7, 15, single)  # 1 fusing callback (and one each of the others)
    for _ in range(TRACE_REPS - 1):
        s.disparity_2(f)
    torch.cuda.synchronize()
    print(f"trace run: single_launch {single}: {TRACE_REPS} x fusing disparity_2, 1 x each other callback")
    s.close()


def kernel_stats(directory):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    print(f"kernels of one rocprofv3 --kernel-trace --stats run of --trace-run ({TRACE_REPS} x fusing disparity_2):")
    with open(paths[0]) as fh:
        for row in csv.DictReader(fh):
            print(f"  {int(row.get('Calls', 0)):5d} calls  avg {float(row.get('AverageNs', 0)) / 1e3:8.2f} us  {row.get('Name', '')[:100]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="write the table here as well")
    ap.add_argument("--trace-run", type=int, choices=(0, 1))
    ap.add_argument("--kernel-stats", metavar="DIR")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        if args.trace_run is not None:
            return trace_run(ctx, args.trace_run)
        lines = []
        bench(ctx, lines)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
