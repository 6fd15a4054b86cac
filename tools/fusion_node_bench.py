#!/usr/bin/env python3
"""Time d2pc_colorize_device and the FusionNode session (the depth_map_fusion node on the device).  GPU only.

Colorize kernel: us and GB/s of algorithmic bytes (1 byte in, 1 + 3 out per view pixel), against two yardsticks timed
in the same process on the same device: (1) Context.membench_copy moving the same number of bytes, (2) the only way
to get these bytes without the kernel: rotate_cw_device + slice + a torch gather table[view.long()] + the gray copy.
Session: us per callback, eager and as a captured graph, at the reference geometry (752 x 480, offsets -7 / 15) for
batch 1 and 16.  The shader clock is sampled beside every timed run (disparity_to_point_cloud_amd/telemetry.py).

  python tools/fusion_node_bench.py [--json PATH]
  python tools/fusion_node_bench.py --trace-run        # 10 x each callback and nothing else: the program for
      rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/fusion_node_bench.py --trace-run
  python tools/fusion_node_bench.py --kernel-stats DIR # kernel names and calls of that run, per callback
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import disparity_to_point_cloud_amd as d2pc  # noqa: E402
from disparity_to_point_cloud_amd import telemetry  # noqa: E402

# (label, frames, rows, cols, (offset_x, offset_y), rotated)
CASES = [("752x480 view 465^2", 1, 480, 752, (-7, 15), False), ("752x480 view 465^2", 1, 480, 752, (-7, 15), True),
         ("752x480 view 465^2", 64, 480, 752, (-7, 15), False), ("752x480 view 465^2", 64, 480, 752, (-7, 15), True),
         ("1080^2 of 1920x1080", 32, 1080, 1920, (0, 0), False), ("1080^2 of 1920x1080", 32, 1080, 1920, (0, 0), True),
         ("2160^2 of 3840x2160", 16, 2160, 3840, (0, 0), False), ("2160^2 of 3840x2160", 16, 2160, 3840, (0, 0), True)]
TRACE_REPS = 10


def timed(fn, iters=20, rounds=7):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1) / iters * 1e3)
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def sampled(card, fn, **kw):
    with telemetry.Sampler(card) as smp:
        med, lo, hi = timed(fn, **kw)
    return med, lo, hi, smp.summary().get("sclk_MHz", {}).get("median")


def bench_colorize(ctx, card, rows_out):
    stream = torch.cuda.current_stream().cuda_stream
    table_t = torch.from_numpy(d2pc.colorize_table()).cuda()
    for label, f, h, w, (ox, oy), rot in CASES:
        x, y, n = d2pc.crop_to_square(h, w, -ox, -oy, oy) if rot else d2pc.crop_to_square(w, h, ox, oy)
        frames = torch.randint(0, 256, (f, h, w), dtype=torch.uint8, device="cuda")
        rgb = torch.empty((f, n, n, 3), dtype=torch.uint8, device="cuda")
        gray = torch.empty((f, n, n), dtype=torch.uint8, device="cuda")
        d = d2pc.colorize_desc_init()
        d.rotate_cw, d.cols, d.rows, d.n_frames = int(rot), w, h, f
        d.x, d.y, d.w, d.h = x, y, n, n
        d.src, d.src_pitch, d.src_frame_stride = frames.data_ptr(), w, w * h
        d.gray, d.gray_pitch, d.gray_frame_stride = gray.data_ptr(), n, n * n
        d.rgb, d.rgb_pitch, d.rgb_frame_stride = rgb.data_ptr(), 3 * n, 3 * n * n
        iters = 20 if f > 1 else 200
        med, lo, hi, sclk = sampled(card, lambda: ctx.colorize_device(d, stream), iters=iters)
        moved = 5 * f * n * n  # bytes: 1 read, 4 written
        # yardstick 1: a copy that moves as many bytes (half read, half written)
        half = (moved // 2 + 255) // 256 * 256
        a, b = torch.empty(half, dtype=torch.uint8, device="cuda"), torch.empty(half, dtype=torch.uint8, device="cuda")
        cmed, _, _, _ = sampled(card, lambda: ctx.membench_copy(a.data_ptr(), b.data_ptr(), half, stream), iters=iters)
        del a, b
        # yardstick 2: the composition available without the kernel
        rotbuf = torch.empty((f, w, h), dtype=torch.uint8, device="cuda") if rot else None

        def composed():
            src = frames
            if rot:
                ctx.rotate_cw_device(frames.data_ptr(), w, h, w, w * h, f, rotbuf.data_ptr(), h, w * h, stream)
                src = rotbuf
            view = src[:, y:y + n, x:x + n]
            return table_t[view.long()], view.contiguous()

        r2, g2 = composed()
        ctx.colorize_device(d, stream)
        torch.cuda.synchronize()
        assert torch.equal(r2, rgb) and torch.equal(g2, gray)
        del r2, g2
        pmed, _, _, _ = sampled(card, composed, iters=max(iters // 4, 5), rounds=5)
        row = {"case": label, "frames": f, "n": n, "rotate_cw": rot, "us": round(med, 2), "us_min": round(lo, 2),
               "us_max": round(hi, 2), "moved_MB": round(moved / 1e6, 2), "GB_s": round(moved / med / 1e3, 1),
               "copy_us": round(cmed, 2), "copy_GB_s": round(2 * half / cmed / 1e3, 1),
               "ratio_to_copy": round((moved / med) / (2 * half / cmed), 3),
               "composition_us": round(pmed, 2), "speedup_vs_composition": round(pmed / med, 2), "sclk_MHz": sclk}
        rows_out.append(row)
        print(f"colorize {label:20s} x{f:3d} {'rot' if rot else '   '}: {med:8.2f} us (min {lo:8.2f}, max {hi:8.2f}) "
              f"{row['moved_MB']:7.2f} MB {row['GB_s']:7.1f} GB/s | copy {cmed:8.2f} us {row['copy_GB_s']:7.1f} GB/s "
              f"ratio {row['ratio_to_copy']:.3f} | rotate+slice+gather {pmed:9.2f} us ({row['speedup_vs_composition']:.1f}x) "
              f"| sclk {sclk} MHz", flush=True)
        del frames, rgb, gray, rotbuf


def make_session(ctx, batch):
    rows, cols = 480, 752
    node = d2pc.FusionNode(ctx, cols, rows, -7, 15, batch=batch)
    shape = (rows, cols) if batch == 1 else (batch, rows, cols)
    fr = {k: torch.randint(0, 256, shape, dtype=torch.uint8, device="cuda") for k in ("D1", "D2", "S1", "S2")}
    calls = {"D1": node.disparity_1, "D2": node.disparity_2, "S1": node.matching_score_1, "S2": node.matching_score_2}
    for k in ("D1", "S1", "S2", "D2"):
        calls[k](fr[k])
    torch.cuda.synchronize()
    return node, fr, calls


def bench_session(ctx, card, rows_out):
    for batch in (1, 16):
        node, fr, calls = make_session(ctx, batch)
        for k in ("D1", "D2", "S1", "S2"):
            med, lo, hi, sclk = sampled(card, lambda: calls[k](fr[k]), iters=50)
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                calls[k](fr[k])
            torch.cuda.current_stream().wait_stream(s)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                calls[k](fr[k])
            gmed, glo, ghi, _ = sampled(card, g.replay, iters=50)
            row = {"session": "752x480 -7/15", "batch": batch, "callback": calls[k].__name__, "eager_us": round(med, 2),
                   "eager_min": round(lo, 2), "eager_max": round(hi, 2), "graph_us": round(gmed, 2),
                   "graph_min": round(glo, 2), "graph_max": round(ghi, 2), "sclk_MHz": sclk}
            rows_out.append(row)
            print(f"session batch {batch:2d} {calls[k].__name__:17s}: eager {med:8.2f} us (min {lo:8.2f}, max {hi:8.2f})  "
                  f"graph {gmed:8.2f} us (min {glo:8.2f}, max {ghi:8.2f})  sclk {sclk} MHz", flush=True)
            del g


def trace_run(ctx):
    """TRACE_REPS x each callback, fused state ready: the launch budget shows as calls per kernel name."""
    node, fr, calls = make_session(ctx, 1)   # 1 x each callback (D2 fusing)
    for k in ("D1", "S1", "S2", "D2"):
        for _ in range(TRACE_REPS - 1):
            calls[k](fr[k])
    torch.cuda.synchronize()
    print(f"trace run: {TRACE_REPS} x disparity_1, matching_score_1, matching_score_2, disparity_2 (fusing)")


def kernel_stats(directory):
    paths = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not paths:
        raise SystemExit(f"no *kernel_stats.csv under {directory}")
    want = {"k_colorize<false>": "disparity_1 (1) + the /gradient colouring of disparity_2 (1)",
            "k_colorize<true>": "disparity_2: rotated view + colouring (1)", "k_fuse_median3": "disparity_2: fuse + median + crop (1)",
            "k_rotate_cw": "matching_score_2: rotate (1)", "k_score_filter": "matching_score_1 (1) + matching_score_2 (1)"}
    print(f"kernels of one rocprofv3 --kernel-trace --stats run of --trace-run ({TRACE_REPS} x each callback):")
    with open(paths[0]) as fh:
        for row in csv.DictReader(fh):
            name, calls = row.get("Name", ""), int(row.get("Calls", 0))
            note = next((v for k, v in want.items() if k in name), "torch (set-up of the run)")
            print(f"  {calls:5d} calls  avg {float(row.get('AverageNs', 0)) / 1e3:8.2f} us  {name[:90]}  <- {note}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="write the rows here as well")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-stats", metavar="DIR")
    args = ap.parse_args()
    if args.kernel_stats:
        return kernel_stats(args.kernel_stats)
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        if args.trace_run:
            return trace_run(ctx)
        card = telemetry.find_card(pci_address=telemetry.torch_pci_address(0))
        colorize_rows, session_rows = [], []
        bench_colorize(ctx, card, colorize_rows)
        bench_session(ctx, card, session_rows)
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "colorize": colorize_rows, "session": session_rows}, fh, indent=1)


if __name__ == "__main__":
    main()
