#!/usr/bin/env python3
"""Time d2pc_score_filter_device (the matching-score pre-filter of MatchingScoreCb1/2: G13 -> Sobel -> threshold ->
G21 -> score + 2 G21) on batches of 8-bit frames, with the shader clock sampled beside every timed run
(disparity_to_point_cloud_amd/telemetry.py), and the one-core numpy restatement (tests/score_filter_ref.py) on one
752 x 480 frame for comparison.  Gpixel/s counts OUTPUT pixels (f * n * n).  GPU only.

  python tools/score_filter_bench.py [--json PATH]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import disparity_to_point_cloud_amd as d2pc  # noqa: E402
from disparity_to_point_cloud_amd import telemetry  # noqa: E402
from disparity_to_point_cloud_amd.torch_api import score_filter  # noqa: E402
import score_filter_ref as ref  # noqa: E402

# (label, frames, height, width, launch offsets of crop_to_square)
CASES = [("752x480 camera", 1, 480, 752, (-7, 15)), ("752x480 camera", 64, 480, 752, (-7, 15)),
         ("1920x1080", 32, 1080, 1920, (0, 0)), ("3840x2160", 16, 2160, 3840, (0, 0))]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--json", help="write the rows here as well")
    args = ap.parse_args()
    card = telemetry.find_card(pci_address=telemetry.torch_pci_address(0))
    rows = []
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        stream = torch.cuda.current_stream().cuda_stream
        for label, f, h, w, (ox, oy) in CASES:
            sq = d2pc.crop_to_square(w, h, ox, oy)
            n = sq[2]
            frames = torch.randint(0, 256, (f, h, w), dtype=torch.uint8, device="cuda")
            for direction, form in ((0, 4), (1, 4), (0, 3)):
                desc = d2pc.score_filter_desc_init()
                desc.direction, desc.form, desc.width, desc.height, desc.n_frames = direction, form, w, h, f
                desc.x, desc.y, desc.n = sq
                desc.src, desc.src_pitch, desc.src_frame_stride = frames.data_ptr(), w, w * h
                out = torch.empty((f, n, n), dtype=torch.uint8, device="cuda")
                desc.out, desc.out_pitch, desc.out_frame_stride = out.data_ptr(), n, n * n
                with telemetry.Sampler(card) as smp:
                    med, lo, hi = timed(lambda: ctx.score_filter_device(desc, stream))
                tel = smp.summary()
                sclk = tel.get("sclk_MHz", {}).get("median")
                px = f * n * n
                row = {"case": label, "frames": f, "n": n, "direction": direction, "form": form, "us": round(med, 1),
                       "us_min": round(lo, 1), "us_max": round(hi, 1), "gpix_s": round(px / med / 1e3, 2),
                       "sclk_MHz": sclk, "power_W": tel.get("power_W", {}).get("median")}
                rows.append(row)
                print(f"{label:15s} x{f:3d} n={n:4d} dir={direction} form=CV{form}: {med:8.1f} us "
                      f"(min {lo:7.1f}, max {hi:7.1f})  {px / med / 1e3:7.2f} Gpix/s  sclk {sclk} MHz", flush=True)
            del frames
    # one-core numpy restatement, one camera frame
    frame = np.random.default_rng(0).integers(0, 256, size=(480, 752)).astype(np.uint8)
    sq = d2pc.crop_to_square(752, 480, -7, 15)
    ts = []
    for _ in range(5):
        t0 = time.perf_counter()
        ref.score_filter(frame, sq, 0, 4)
        ts.append((time.perf_counter() - t0) * 1e6)
    cpu = float(np.median(ts))
    rows.append({"case": "752x480 camera, numpy restatement (one CPU core)", "frames": 1, "n": sq[2], "direction": 0,
                 "form": 4, "us": round(cpu, 1), "gpix_s": round(sq[2] ** 2 / cpu / 1e3, 4)})
    print(f"numpy restatement, one 752x480 frame (n={sq[2]}): {cpu:10.1f} us  {sq[2] ** 2 / cpu / 1e3:.4f} Gpix/s")
    if args.json:
        with open(args.json, "w") as fh:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
