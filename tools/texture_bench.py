#!/usr/bin/env python3
"""What a textured cloud costs behind its producer, interleaved in ONE process on ONE device (tools/ab.py's method: the
arms take turns round by round; devices and runs differ by ~10 %, so nothing else ranks them).  GPU box only.

  A  the producer alone (d2pc_process_device / d2pc_rig_process_device): what a caller had before
  B  the producer + d2pc_texture_device behind it, on one stream
  T  d2pc_texture_device alone, on the cloud the producer left
  C  d2pc_membench_copy (d2pc_ext.h) of as many bytes as T moves (read + written, so a copy of half of them), in the
     same run: what this device gives a kernel that only streams

  python tools/texture_bench.py            ->  profiles/texture_bench.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import disparity_to_point_cloud_amd as d2pc  # noqa: E402

# (name, cameras, w, h, mode, rig, index, holes)
CASES = [("1 x 752x480 u8 COMPACT", 1, 752, 480, d2pc.MODE_COMPACT, False, True, 0.3),
         ("16 x 752x480 u8 rig merged COMPACT", 16, 752, 480, d2pc.MODE_COMPACT, True, True, 0.3),
         ("16 x 3840x2160 u8 PARITY no index", 16, 3840, 2160, d2pc.MODE_PARITY, False, False, 0.0)]
BORDER = 40


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
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "texture_bench.txt"))
    a = ap.parse_args()
    prop = torch.cuda.get_device_properties(0)
    lines = ["# tools/texture_bench.py --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs, %.0f GiB (one device, one process; arms interleaved round by round)" % (
                 prop.name, prop.multi_processor_count, prop.total_memory / 2**30),
             "# A = producer alone; B = producer + d2pc_texture_device; T = d2pc_texture_device alone; C = d2pc_membench_copy of the bytes T moves",
             "# 8-bit texture (the camera image / COMBINED_SCORE) -> PointXYZI; us per call: median (min .. max) over the rounds;",
             "# a timed window is --iters calls or as many as fill ~30 ms, whichever is more",
             "# T moves per point: 16 B point + 4 B index (none in the PARITY layout) + 1 B sample read, 32 B written",
             "%-36s %10s %9s %-30s %-30s %-30s %-30s %8s %6s %6s" % (
                 "case", "points", "MB moved", "A", "B", "T", "C", "B-A", "C/T", "T GB/s")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    for name, n, w, h, mode, rig_case, want_index, holes in CASES:
        frames = torch.randint(8, 256, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
        if holes:
            frames[torch.rand((n, h, w), generator=gen, device="cuda") < holes] = 0
        image = torch.randint(0, 256, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
        roi_n = d2pc.roi_points(w, h, BORDER)
        cap = n * roi_n
        pts = torch.empty((cap, 4), dtype=torch.float32, device="cuda")
        idx = torch.empty((cap,), dtype=torch.int32, device="cuda") if want_index else None
        out = torch.empty((cap, 8), dtype=torch.float32, device="cuda")
        counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        ip = idx.data_ptr() if want_index else None
        qs = [d2pc.make_q(fx=714.24 - 3.0 * f, fy=713.5 - 3.0 * f, cx=376.0 + f, cy=240.0 - f) for f in range(n)]
        with d2pc.Context(q=qs[0], border=BORDER, mode=mode) as ctx:
            rig = d2pc.RigSession(ctx, n, w, h, d2pc.DTYPE_U8, qs) if rig_case else None
            desc = d2pc.texture_desc_init(
                width=w, height=h, border=BORDER, n_frames=n, merged=int(rig_case), texture=image.data_ptr(), tex_pitch=w,
                tex_frame_stride=w * h, points=pts.data_ptr(), index=ip,
                counts=(offsets.data_ptr() + 4 * n) if rig_case else counts.data_ptr(),
                cloud_points=cap if rig_case else roi_n, points_frame_stride_points=roi_n, out=out.data_ptr(),
                out_frame_stride_points=roi_n)

            def produce():
                if rig_case:
                    rig.process_device(frames.data_ptr(), 0.125, w, h * w, pts.data_ptr(), ip, cap, counts.data_ptr(),
                                       offsets.data_ptr(), s)
                else:
                    ctx.process_device(frames.data_ptr(), d2pc.DTYPE_U8, 0.125, w, h, w, h * w, n, pts.data_ptr(), ip, roi_n,
                                       counts.data_ptr(), s)

            def attach():
                ctx.texture_device(desc, s)

            def both():
                produce()
                attach()

            both()
            torch.cuda.synchronize()
            ctx.check_async_error()
            npts = int(counts.cpu().numpy().view(np.uint32).sum())
            moved = (16 + (4 if want_index else 0) + 1 + 32) * npts
            half = max(moved // 2 // 16 * 16, 16)
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")

            def copy():
                ctx.membench_copy(src.data_ptr(), dst.data_ptr(), half, s)

            arms = (produce, both, attach, copy)
            for fn in arms:   # warm-up: allocations, code objects
                fn()
            torch.cuda.synchronize()
            # a timed window of at least ~30 ms: small cases take more iterations
            iters = int(min(max(a.iters, 30000.0 / timed(both, 5)), 4000))
            t = [[] for _ in arms]
            for r in range(a.rounds):
                for k in range(len(arms)):
                    k2 = (k + r) % len(arms)   # the order rotates too
                    t[k2].append(timed(arms[k2], iters))
            ctx.check_async_error()
            if rig is not None:
                rig.close()
        ma, mb, mt, mc = (float(np.median(x)) for x in t)
        lines.append("%-36s %10d %9.1f %-30s %-30s %-30s %-30s %8.1f %6.2f %6.0f" % (
            name, npts, moved / 1e6, fmt(t[0]), fmt(t[1]), fmt(t[2]), fmt(t[3]), mb - ma, mc / mt, moved / mt / 1e3))
        print(lines[-1], flush=True)
        del frames, image, pts, idx, out, src, dst
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
