#!/usr/bin/env python3
"""What the obstacle sectors (include/d2pc_sectors.h) cost behind their producer, interleaved in ONE process on ONE
device (tools/ab.py's method: the arms take turns round by round; devices and runs differ by ~10 %, so nothing else
ranks them).  GPU box only.

  A   the producer alone (d2pc_process_device / d2pc_rig_process_device)
  B   the producer + d2pc_sectors_process_device behind it, on one stream
  S   d2pc_sectors_process_device alone, on the cloud the producer left (two launches)
  S0  the same call with every count 0: what the two launches cost before the first record (the blocks' tables are
      initialised and stored as slabs, the finishing kernel does all of its work)
  C   d2pc_membench_copy (d2pc_ext.h) that moves as many bytes as S reads (a copy of half of them: read + written), in
      the same run: what this device gives a kernel that only streams.  There is no earlier time to compare with.
  CPU tests/sectors_ref.py (numpy, one core) on the first million points of the cloud, per million points

  python tools/sectors_bench.py         ->  profiles/sectors_bench.txt
  python tools/sectors_bench.py --ab    ->  profiles/sectors_ab.txt: the wave pre-reduction against plain per-lane LDS atomics
                                            (`make sectors SNAME=wave SDEFS=-DD2PC_SECTORS_FORCE_ROUNDS=2`, `... SNAME=plain
                                            SDEFS=-DD2PC_SECTORS_FORCE_ROUNDS=0`; the product picks by the grid's size), on a
                                            cloud in producer order and on the same cloud shuffled, for the smallest and the
                                            largest grid
  python tools/sectors_bench.py --elevation [--parent NAME]
                                        ->  profiles/sectors_elevation_bench.txt: elevation layers (layer_kind 1) beside height
                                            layers on the rig's merged cloud, S / S0 / C of 72 x 16 height, 72 x 16 elevation and
                                            60 x 30 elevation in ONE interleaved run; with --parent NAME also the height rows
                                            72 x 1 and 360 x 16 of this build against libd2pc_sectors_NAME.so, a build of the
                                            sources before the elevation layers (`make sectors SNAME=NAME` there): the height
                                            instantiation may not be slower than it by more than the arms' spread
  python tools/sectors_bench.py --memory
                                        ->  profiles/sectors_memory_bench.txt: the memory (d2pc_sectors_memory_update_device, one
                                            launch of one block) behind the sectors: M = the update alone, SM = the sectors call +
                                            the update, beside S and S0 of the same session, on the one-camera frame and on the
                                            rig's merged cloud, for 72 x 1 and 60 x 30 elevation, in ONE interleaved run.  No time
                                            is fixed in advance: the yardstick is S0, the sectors' own fixed part, in the same run
  python tools/sectors_bench.py --parent NAME
                                        ->  profiles/sectors_refactor_bench.txt: this build against libd2pc_sectors_NAME.so, a build
                                            of the parent commit's sources (`make sectors SNAME=NAME` there), when a change must move
                                            neither a byte nor the time: S of 72 x 1, 360 x 16 height, 72 x 16 and 60 x 30 elevation
                                            and M of 72 x 1 and 60 x 30 elevation on the rig's merged cloud, the steer's T and T32 of
                                            72 x 1 and 60 x 30 elevation, the ground's G of 16 x 16 and 64 x 64 cells and the terrain's
                                            update U of 16 x 16 x 8 and 64 x 64 x 16 on the rig's level ground, the outputs of the two
                                            builds compared bit for bit first, all arms in ONE interleaved run; a row's new median may
                                            exceed the parent's by no more than the arms' spread in that run
  python tools/sectors_bench.py --steer [--parent NAME]
                                        ->  profiles/sectors_steer_bench.txt: the steer (d2pc_sectors_steer_device, one launch of one
                                            block) behind the sectors and the memory: T = the steer alone (T32: 32 candidates), SMT =
                                            the sectors call + the update + the steer, beside S0, M and SM of the same sessions, on the
                                            one-camera frame and on the rig's merged cloud, for 72 x 1 and 60 x 30 elevation, in ONE
                                            interleaved run.  No time is fixed in advance: the yardsticks are S0 and M of the same run.
                                            With --parent NAME also T and T32 of libd2pc_sectors_NAME.so, another build of the steer's
                                            kernel, its outputs compared bit for bit with this build's first
  python tools/sectors_bench.py --ground
                                        ->  profiles/sectors_ground_bench.txt: the landing grid (d2pc_sectors_ground_process_device, three
                                            launches) on a level ground under a camera that looks down: G = the call alone, G0 = with a
                                            count of 0 (the fixed part), C = the copy of the bytes G reads, S / S0 = the 72 x 1 sectors call
                                            on the same cloud, for 16 x 16 and 64 x 64 cells, the one-camera frame and the rig's merged
                                            cloud, in producer order and shuffled, in ONE interleaved run
  python tools/sectors_bench.py --terrain
                                        ->  profiles/sectors_terrain_bench.txt: the terrain's update (d2pc_sectors_terrain_update_device,
                                            one launch of one block) alone on the ground call's tables, for 16 x 16 cells at depth 8 and
                                            64 x 64 at depth 16, with every slot of the window taking part and with none, beside the ground
                                            call's G and G0 and the steer call on the same one-camera cloud, in ONE interleaved run.  No
                                            time is fixed in advance: T is read against G0 and G of its row
  python tools/sectors_bench.py --slope
                                        ->  profiles/sectors_slope_bench.txt: the plane fit per cell (d2pc_sectors_slope_process_device,
                                            three launches, ten LDS adds a record and slabs of 76 bytes a cell) beside the ground call of
                                            the same configuration (three adds, 20 bytes): L = the slope call, L0 = with a count of 0, G and
                                            G0 = the ground's, C = the copy of the bytes they read, for 16 x 16 and 46 x 46 cells, the
                                            one-camera frame and the rig's merged cloud, in producer order and shuffled, in ONE interleaved
                                            run.  No time is fixed in advance: L is read against G and C of its row; L0 - G0 is what the
                                            larger slabs cost, (L - L0) - (G - G0) what the seven more adds a record cost
  python tools/sectors_bench.py --relief
                                        ->  profiles/sectors_relief_bench.txt: the relief's update (d2pc_sectors_relief_update_device, two launches,
                                            stored tables of 76 bytes a cell) alone at 16 x 16 x 8 and 46 x 46 x 16, with every slot of the window
                                            taking part and with none, beside the slope call's L and L0, the terrain's update of the same grid and
                                            depth and a copy of the bytes the update reads, in ONE interleaved run.  No time is fixed in advance
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import disparity_to_point_cloud_amd as d2pc  # noqa: E402
import sectors_ref  # noqa: E402

# (name, cameras, w, h, mode, rig, holes)
CASES = [("1 x 752x480 u8 COMPACT", 1, 752, 480, d2pc.MODE_COMPACT, False, 0.3),
         ("16 x 752x480 u8 rig merged COMPACT", 16, 752, 480, d2pc.MODE_COMPACT, True, 0.3),
         ("16 x 3840x2160 u8 PARITY", 16, 3840, 2160, d2pc.MODE_PARITY, False, 0.0)]
BORDER = 40
CPU_POINTS = 1_000_000


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


def yaw(deg):
    a = np.deg2rad(deg)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)   # about the optical frame's y
    return m


def interleaved(arms, rounds, iters):
    t = [[] for _ in arms]
    for r in range(rounds):
        for k in range(len(arms)):
            k2 = (k + r) % len(arms)   # the order rotates too
            t[k2].append(timed(arms[k2], iters))
    return t


class Producer:
    """One case's frames, cloud buffers and the call that fills them."""

    def __init__(self, ctx, n, w, h, rig_case, holes, gen):
        self.n, self.rig_case = n, rig_case
        self.frames = torch.randint(8, 256, (n, h, w), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
        if holes:
            self.frames[torch.rand((n, h, w), generator=gen, device="cuda") < holes] = 0
        self.roi_n = d2pc.roi_points(w, h, BORDER)
        self.cap = n * self.roi_n
        self.pts = torch.empty((self.cap, 4), dtype=torch.float32, device="cuda")
        self.counts = torch.zeros(n, dtype=torch.int32, device="cuda")
        self.offsets = torch.zeros(n + 1, dtype=torch.int32, device="cuda")
        q = d2pc.make_q()
        qs = [d2pc.rig_compose_q(yaw(360.0 * f / n), q) for f in range(n)]   # the cameras look all round
        self.rig = d2pc.RigSession(ctx, n, w, h, d2pc.DTYPE_U8, qs) if rig_case else None
        self.ctx, self.w, self.h = ctx, w, h

    def __call__(self, s):
        if self.rig_case:
            self.rig.process_device(self.frames.data_ptr(), 0.125, self.w, self.h * self.w, self.pts.data_ptr(), None, self.cap,
                                    self.counts.data_ptr(), self.offsets.data_ptr(), s)
        else:
            self.ctx.process_device(self.frames.data_ptr(), d2pc.DTYPE_U8, 0.125, self.w, self.h, self.w, self.h * self.w, self.n,
                                    self.pts.data_ptr(), None, self.roi_n, self.counts.data_ptr(), s)

    def cloud(self):
        """What the sectors call gets: (n_clouds, cloud_points, stride, counts pointer)."""
        if self.rig_case:
            return 1, self.cap, 0, self.offsets.data_ptr() + 4 * self.n
        return self.n, self.roi_n, self.roi_n, self.counts.data_ptr()

    def close(self):
        if self.rig is not None:
            self.rig.close()


# ---- the inputs --steer, --ground, --terrain and --parent share
HALF_PI = float(np.float32(np.pi / 2))
HISTOGRAM = dict(n_sectors=60, n_layers=30, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60, layer_kind=d2pc.LAYERS_ELEVATION)
# (row, grid, the steer's reach)
STEER_GRIDS = [("72 x 1", dict(), dict(max_reach_sectors=8, max_reach_layers=0)),
               ("60 x 30 elevation", HISTOGRAM, dict(max_reach_sectors=8, max_reach_layers=4))]
GROUND_GRIDS = [(dict(n_a=16, n_b=16, cell_size=0.5), 8), (dict(n_a=64, n_b=64, cell_size=0.125), 16)]   # (grid, the terrain's depth)
NADIR = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])


def steer_outputs(n_cells, k):
    return dict(clearance_cm=torch.empty(n_cells, dtype=torch.int16, device="cuda"), cost=torch.empty(n_cells, dtype=torch.int32, device="cuda"),
                candidates=torch.empty(k, dtype=torch.int64, device="cuda"), summary=torch.empty(4, dtype=torch.int32, device="cuda"))


def ground_outputs(nc, k):
    return dict(count=torch.empty(nc, dtype=torch.int32, device="cuda"), sum=torch.empty(nc, dtype=torch.int64, device="cuda"),
                sum2=torch.empty(nc, dtype=torch.int64, device="cuda"), mean_q=torch.empty(nc, dtype=torch.int32, device="cuda"),
                spread_q2=torch.empty(nc, dtype=torch.int32, device="cuda"), flat=torch.empty(nc, dtype=torch.uint8, device="cuda"),
                site=torch.empty(nc, dtype=torch.uint8, device="cuda"), candidates=torch.empty(k, dtype=torch.int64, device="cuda"),
                summary=torch.empty(4, dtype=torch.int32, device="cuda"))


def ground_grid(grid, prod):
    """A ground configuration of the level-ground cloud: flat up to a standard deviation of 0.15 m, steps up to 100 quanta."""
    return dict(grid, max_points=prod.cap, max_spread_q2=d2pc.sectors_ground_spread_of_std(0.002, 0.15), max_step_q=100)


def level_ground(ctx, prod, gen, s):
    """The producer's frames replaced by a level ground 5.4 m below a camera that looks straight down (its holes kept) and
    run -> (records, the cloud, the grid's corner: 4 m to either side of camera 0's median record, h0 at its median height)."""
    level = torch.randint(94, 99, tuple(prod.frames.shape), generator=gen, device="cuda", dtype=torch.int32).to(torch.uint8)
    level[prod.frames == 0] = 0
    prod.frames = level
    prod(s)
    torch.cuda.synchronize()
    ctx.check_async_error()
    npts = int(prod.offsets.cpu().numpy().view(np.uint32)[prod.n]) if prod.rig_case else int(prod.counts.cpu().numpy().view(np.uint32)[0])
    cloud = prod.pts[:npts].clone()
    mid = np.median(cloud[:min(npts, prod.roi_n // 2), :3].cpu().numpy().astype(np.float64) @ NADIR.T + [0.0, 0.0, 10.0], axis=0)
    return npts, cloud, [np.round(mid[0]) - 4.0, np.round(mid[1]) - 4.0, float(np.float32(mid[2]))]   # a multiple of both cell sizes


def ground_step(corner):
    """The nadir pose and the grid's corner as a device step, the goal on cell (8, 8)."""
    return torch.from_numpy(d2pc.sectors_ground_step(NADIR, [0.0, 0.0, 10.0], corner, 8, 8).view(np.int32).copy()).to("cuda")


def bench(a):
    prop = torch.cuda.get_device_properties(0)
    lines = ["# tools/sectors_bench.py --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs, %.0f GiB (one device, one process, ONE run; arms interleaved round by round)" % (
                 prop.name, prop.multi_processor_count, prop.total_memory / 2**30),
             "# A = producer alone; B = producer + sectors; S = sectors alone (two launches); S0 = sectors with every count 0;",
             "# C = d2pc_membench_copy moving the bytes S reads (16 B per point); the default grid: 72 sectors x 1 layer, all four outputs",
             "# us per call: median (min .. max) over the rounds; a timed window is --iters calls or as many as fill ~30 ms",
             "# CPU = tests/sectors_ref.py (numpy, one core) on the cloud's first %d points, ms per million points" % CPU_POINTS,
             "%-36s %10s %8s %-30s %-30s %-30s %-30s %-30s %8s %6s %7s %9s" % (
                 "case", "points", "MB read", "A", "B", "S", "S0", "C", "B-A", "S/C", "S GB/s", "CPU ms/M")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    for name, n, w, h, mode, rig_case, holes in (CASES if a.only is None else CASES[a.only:a.only + 1]):
        with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx, d2pc.Sectors() as sec:
            prod = Producer(ctx, n, w, h, rig_case, holes, gen)
            n_clouds, cp, stride, counts_ptr = prod.cloud()
            out = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"),
                       count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"),
                       nearest=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"),
                       distance_cm=torch.empty(sec.n_cells, dtype=torch.int16, device="cuda"))
            zeros = torch.zeros(n_clouds, dtype=torch.int32, device="cuda")

            def produce():
                prod(s)

            def sectors():
                sec.process(prod.pts, cp, n_clouds=n_clouds, counts=counts_ptr, frame_stride_points=stride, stream_ptr=s, **out)

            def empty():
                sec.process(prod.pts, cp, n_clouds=n_clouds, counts=zeros, frame_stride_points=stride, stream_ptr=s, **out)

            def both():
                produce()
                sectors()

            both()
            torch.cuda.synchronize()
            ctx.check_async_error()
            cn = prod.counts.cpu().numpy().view(np.uint32)
            npts = int(cn.sum())
            assert int(out["count"].cpu().numpy().view(np.uint32).sum()) <= npts
            read = 16 * npts
            half = max(read // 2 // 16 * 16, 16)
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")

            def copy():
                ctx.membench_copy(src.data_ptr(), dst.data_ptr(), half, s)

            arms = (produce, both, sectors, empty, copy)
            for fn in arms:   # warm-up: allocations, code objects
                fn()
            torch.cuda.synchronize()
            iters = int(min(max(a.iters, 30000.0 / timed(both, 5)), 4000))
            t = interleaved(arms, a.rounds, iters)
            ctx.check_async_error()
            # the CPU column: the reference on one core, the cloud's first points
            m = min(CPU_POINTS, int(cn[0]) if not rig_case else npts)
            xyz = prod.pts[:m, :3].cpu().numpy()
            ref = sectors_ref.SectorsRef(sec.cfg, d2pc.sectors_table(sec.cfg), sec.geometry)
            t0 = time.perf_counter()
            ref.grid(xyz, np.arange(m))
            cpu = (time.perf_counter() - t0) * 1e3 / (m / 1e6)
            prod.close()
        ma, mb, ms, m0, mc = (float(np.median(x)) for x in t)
        lines.append("%-36s %10d %8.1f %-30s %-30s %-30s %-30s %-30s %8.1f %6.2f %7.0f %9.0f" % (
            name, npts, read / 1e6, fmt(t[0]), fmt(t[1]), fmt(t[2]), fmt(t[3]), fmt(t[4]), mb - ma, ms / mc, read / ms / 1e3, cpu))
        print(lines[-1], flush=True)
        del prod, src, dst
        torch.cuda.empty_cache()
    return lines


def ab(a):
    """The two arms of the in-wave reduction on one cloud, in producer order and shuffled."""
    prop = torch.cuda.get_device_properties(0)
    lines = ["# tools/sectors_bench.py --ab --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; arms interleaved round by round)" % (prop.name, prop.multi_processor_count),
             "# wave = libd2pc_sectors_wave.so (-DD2PC_SECTORS_FORCE_ROUNDS=2: two elected cells per wave, then per-lane LDS atomics);",
             "# plain = libd2pc_sectors_plain.so (-DD2PC_SECTORS_FORCE_ROUNDS=0: per-lane LDS atomics only).  S alone, us per call: median (min .. max)",
             "# product = libd2pc_sectors.so: wave up to 72 cells, plain beyond",
             "%-44s %10s %-30s %-30s %-30s %10s" % ("cloud", "points", "wave", "plain", "product", "plain/wave")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    name, n, w, h, mode, rig_case, holes = CASES[1]
    for grid in (dict(), dict(n_sectors=360, n_layers=16, u_min=-40.0, u_max=40.0)):
        with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx, d2pc.Sectors(variant="wave", **grid) as wave, \
                d2pc.Sectors(variant="plain", **grid) as plain, d2pc.Sectors(**grid) as product:
            prod = Producer(ctx, n, w, h, rig_case, holes, gen)
            prod(s)
            torch.cuda.synchronize()
            npts = int(prod.offsets.cpu().numpy().view(np.uint32)[n])
            ordered = prod.pts[:npts].clone()
            shuffled = ordered[torch.randperm(npts, generator=gen, device="cuda")].contiguous()
            outs = [dict(range=torch.empty(wave.n_cells, dtype=torch.float32, device="cuda"),
                         count=torch.empty(wave.n_cells, dtype=torch.int32, device="cuda")) for _ in range(3)]
            for label, cloud in (("producer order", ordered), ("shuffled", shuffled)):
                arms = tuple((lambda sec=sec, o=o: sec.process(cloud, npts, stream_ptr=s, **o)) for sec, o in zip((wave, plain, product), outs))
                for fn in arms:
                    fn()
                torch.cuda.synchronize()
                assert all(torch.equal(outs[0][k], o[k]) for o in outs[1:] for k in o), "the arms disagree"
                iters = int(min(max(a.iters, 30000.0 / timed(arms[0], 5)), 4000))
                t = interleaved(arms, a.rounds, iters)
                lines.append("%-44s %10d %-30s %-30s %-30s %10.2f" % (
                    "%d x %d cells, %s" % (wave.cfg.n_sectors, wave.cfg.n_layers, label), npts, fmt(t[0]), fmt(t[1]), fmt(t[2]),
                    float(np.median(t[1])) / float(np.median(t[0]))))
                print(lines[-1], flush=True)
            prod.close()
    return lines


def elevation(a):
    """Elevation layers beside height layers, and this build's height rows beside an earlier build's."""
    prop = torch.cuda.get_device_properties(0)
    half_pi = float(np.float32(np.pi / 2))
    grids = [("72 x 16 height", dict(n_sectors=72, n_layers=16, u_min=-40.0, u_max=40.0)),
             ("72 x 16 elevation", dict(n_sectors=72, n_layers=16, u_min=-half_pi, u_max=half_pi, layer_kind=d2pc.LAYERS_ELEVATION)),
             ("60 x 30 elevation", dict(n_sectors=60, n_layers=30, u_min=-half_pi, u_max=half_pi, azimuth0=-np.pi / 60,
                                        layer_kind=d2pc.LAYERS_ELEVATION))]
    versus = [("72 x 1 height", dict()), ("360 x 16 height", dict(n_sectors=360, n_layers=16, u_min=-40.0, u_max=40.0))]
    lines = ["# tools/sectors_bench.py --elevation%s --rounds %d --iters %d" % (" --parent " + a.parent if a.parent else "", a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; every arm of this file interleaved round by round)" % (
                 prop.name, prop.multi_processor_count),
             "# the 16-camera rig's merged cloud; S = d2pc_sectors_process_device alone (two launches, range + count); S0 = the same with",
             "# a count of 0; C = d2pc_membench_copy moving the bytes S reads (16 B per point).  us per call: median (min .. max)"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    name, n, w, h, mode, rig_case, holes = CASES[1]
    with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx:
        prod = Producer(ctx, n, w, h, rig_case, holes, gen)
        prod(s)
        torch.cuda.synchronize()
        npts = int(prod.offsets.cpu().numpy().view(np.uint32)[n])
        cloud = prod.pts[:npts].clone()
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        half = max(16 * npts // 2 // 16 * 16, 16)
        src = torch.empty(half, dtype=torch.uint8, device="cuda")
        dst = torch.empty(half, dtype=torch.uint8, device="cuda")
        sessions, arms, labels = [], [lambda: ctx.membench_copy(src.data_ptr(), dst.data_ptr(), half, s)], ["C"]

        def add(label, grid, variant=None, empty=False):
            sec = d2pc.Sectors(variant=variant, **grid)
            out = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"),
                       count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
            sessions.append((sec, out))
            arms.append(lambda: sec.process(cloud, npts, stream_ptr=s, **out))
            labels.append(label)
            if empty:
                arms.append(lambda: sec.process(cloud, npts, counts=zero, stream_ptr=s, **out))
                labels.append(label + " S0")

        for label, grid in grids:
            add(label, grid, empty=True)
        for label, grid in versus if a.parent else []:
            add(label + " new", grid)
            add(label + " parent", grid, variant=a.parent)
        for fn in arms:   # warm-up: code objects
            fn()
        torch.cuda.synchronize()
        if a.parent:   # the two builds compute the same bytes
            for i in range(len(grids), len(sessions), 2):
                assert all(torch.equal(sessions[i][1][k], sessions[i + 1][1][k]) for k in ("range", "count")), "the builds disagree"
        iters = int(min(max(a.iters, 30000.0 / timed(arms[1], 5)), 4000))
        t = dict(zip(labels, interleaved(arms, a.rounds, iters)))
        ctx.check_async_error()
        med = {k: float(np.median(v)) for k, v in t.items()}
        lines.append("# %d points, %.1f MB read, %d calls per timed window" % (npts, 16 * npts / 1e6, iters))
        lines.append("%-20s %8s %10s %-30s %-30s %-30s %6s" % ("grid", "cells", "LDS B", "S", "S0", "C", "S/C"))
        for (label, grid), (sec, _) in zip(grids, sessions):
            lines.append("%-20s %8d %10d %-30s %-30s %-30s %6.2f" % (label, sec.n_cells, sec.geometry.lds_bytes, fmt(t[label]), fmt(t[label + " S0"]),
                                                                   fmt(t["C"]), med[label] / med["C"]))
        if a.parent:
            lines.append("# the height instantiation against libd2pc_sectors_%s.so: new may be slower by no more than the larger of the two arms'" % a.parent)
            lines.append("# (max - min) / median in this run")
            lines += verdicts(t, [label for label, _ in versus])
        for sec, _ in sessions:
            sec.close()
        prod.close()
    for ln in lines:
        print(ln, flush=True)
    return lines


def verdicts(t, rows):
    """The table of `row new` against `row parent` of the timings t: the project's rule for a build against its parent."""
    lines = ["%-24s %-30s %-30s %10s %10s %s" % ("row", "new", "parent", "new/parent", "allowed", "verdict")]
    for row in rows:
        new, old = t[row + " new"], t[row + " parent"]
        spread = max((max(v) - min(v)) / float(np.median(v)) for v in (new, old))
        ratio = float(np.median(new)) / float(np.median(old))
        lines.append("%-24s %-30s %-30s %10.4f %10.4f %s" % (row, fmt(new), fmt(old), ratio, 1.0 + spread, "ok" if ratio <= 1.0 + spread else "SLOWER"))
    return lines


def same_bytes(new, old):
    """Whether two builds' outputs of one row hold the same bytes."""
    bits = lambda x: x.view(torch.int32) if x.dtype == torch.float32 else x  # noqa: E731
    return all(torch.equal(bits(new[k]), bits(old[k])) for k in new)


def parent(a):
    """This build against libd2pc_sectors_<parent>.so: S of four grids and M of two on the rig's merged cloud, T and T32 of
    two grids on the memory's distance_cm, G of two grids and the terrain's update U of two windows on the rig's level
    ground; the outputs of the two builds of every row compared bit for bit first, then all arms interleaved in one run."""
    prop = torch.cuda.get_device_properties(0)
    builds = (("new", None), ("parent", a.parent))
    s_rows = [("S 72 x 1 height", dict()), ("S 360 x 16 height", dict(n_sectors=360, n_layers=16, u_min=-40.0, u_max=40.0)),
              ("S 72 x 16 elevation", dict(n_sectors=72, n_layers=16, u_min=-HALF_PI, u_max=HALF_PI, layer_kind=d2pc.LAYERS_ELEVATION)),
              ("S 60 x 30 elevation", HISTOGRAM)]
    m_rows = [("M 72 x 1 height", STEER_GRIDS[0]), ("M 60 x 30 elevation", STEER_GRIDS[1])]
    lines = ["# tools/sectors_bench.py --parent %s --rounds %d --iters %d" % (a.parent, a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; every arm of this file interleaved round by round)" % (
                 prop.name, prop.multi_processor_count),
             "# new = libd2pc_sectors.so, parent = libd2pc_sectors_%s.so (`make sectors SNAME=%s` of the parent commit's sources), on the" % (a.parent, a.parent),
             "# 16-camera rig's merged cloud.  S = d2pc_sectors_process_device alone (range + count); M = d2pc_sectors_memory_update_device",
             "# alone (range, distance_cm, age; a 37-degree yaw, a translation and dt 50 every call, max_age 2,000, a forward field of",
             "# view as `covered`); T / T32 = d2pc_sectors_steer_device alone (reach 8 sectors and 0 / 4 layers, clearance_cm, cost, summary and",
             "# 1 / 32 candidates) on the distance_cm M's row left behind its warm-up; G = d2pc_sectors_ground_process_device alone (three",
             "# launches, all nine outputs, 32 candidates) on the rig's merged cloud of tools/sectors_bench.py --ground's level ground; U =",
             "# d2pc_sectors_terrain_update_device alone (all nine outputs, 32 candidates, status) on the new G's count / sum / sum2 with the",
             "# corner held: every slot of the window takes part.  The two builds' outputs of every row were compared bit for bit before the",
             "# timing.  us per call: median (min .. max).  new may be slower by no more than the larger of the two arms' (max - min) / median",
             "# in this run"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    name, n, w, h, mode, rig_case, holes = CASES[1]
    with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx:
        prod = Producer(ctx, n, w, h, rig_case, holes, gen)
        prod(s)
        torch.cuda.synchronize()
        ctx.check_async_error()
        npts = int(prod.offsets.cpu().numpy().view(np.uint32)[n])
        cloud = prod.pts[:npts].clone()
        level_n, level_cloud, corner = level_ground(ctx, prod, gen, s)
        g_rows = [(ground_grid(grid, prod), depth) for grid, depth in GROUND_GRIDS]
        prod.close()
    R = np.array([[np.cos(0.6458), 0.0, np.sin(0.6458)], [0.0, 1.0, 0.0], [-np.sin(0.6458), 0.0, np.cos(0.6458)]])   # about the optical y
    step = torch.from_numpy(d2pc.sectors_memory_step(R, [0.4, -0.1, 0.9], 50).view(np.int32).copy()).to("cuda")
    arms, labels, pairs, keep = [], [], [], []

    def add(row, which, fn):
        arms.append(fn)
        labels.append("%s %s" % (row, which))

    for row, grid in s_rows:
        outs = []
        for which, variant in builds:
            sec = d2pc.Sectors(variant=variant, **grid)
            out = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"),
                       count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
            keep.append(sec)
            outs.append(out)
            add(row, which, lambda sec=sec, out=out: sec.process(cloud, npts, stream_ptr=s, **out))
        pairs.append((row, outs))
    memories = []
    for row, (_, grid, reach) in m_rows:
        sec = d2pc.Sectors(**grid)
        seen = dict(count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"),
                    nearest=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
        sec.process(cloud, npts, stream_ptr=s, **seen)
        cov = torch.from_numpy(d2pc.sectors_memory_coverage(sec.cfg, [(0.0, 0.0, 1.5, 1.0, 0.05)])).to("cuda")
        keep += [sec, seen, cov]
        outs = []
        for which, variant in builds:
            mem = d2pc.SectorsMemory(sec.cfg, 2000, variant=variant)
            out = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"),
                       distance_cm=torch.empty(sec.n_cells, dtype=torch.int16, device="cuda"),
                       age=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
            keep.append(mem)
            outs.append(out)
            add(row, which, lambda mem=mem, seen=seen, cov=cov, out=out: mem.update(cloud, npts, seen["count"], seen["nearest"], step, covered=cov,
                                                                                    stream_ptr=s, **out))
        pairs.append((row, outs))
        memories.append((sec, outs[0]))
    for _ in range(3):   # warm-up: code objects; three updates, so that the memories carry, age and drop
        for fn in arms:
            fn()
        torch.cuda.synchronize()
        for row, (new, old) in pairs:   # (the memories of the two builds advance in step: the same number of calls)
            assert same_bytes(new, old), row + ": the builds disagree"
    # ---- the one-block kernels and the ground: T on a copy of what M left (M goes on advancing), G and U on the level ground
    first = len(arms)
    for (gname, _, reach), (sec, left) in zip(STEER_GRIDS, memories):
        dcm = left["distance_cm"].clone()
        goal = torch.from_numpy(d2pc.sectors_steer_step(sec.cfg.n_sectors // 3, sec.cfg.n_layers // 2, 1, sec.cfg.n_layers // 2)
                                .view(np.int32).copy()).to("cuda")
        keep += [dcm, goal]
        for tag, k in (("T", 1), ("T32", 32)):
            row, outs = "%s %s" % (tag, gname), []
            for which, variant in builds:
                st = d2pc.SectorsSteer(sec.cfg, variant=variant, **reach)
                out = steer_outputs(sec.n_cells, k)
                keep.append(st)
                outs.append(out)
                add(row, which, lambda st=st, dcm=dcm, goal=goal, k=k, out=out: st.steer(dcm, goal, n_candidates=k, stream_ptr=s, **out))
            pairs.append((row, outs))
    gstep = ground_step(corner)
    count = torch.tensor([level_n], dtype=torch.int32, device="cuda")
    windows = []
    for grid, depth in g_rows:
        row, outs = "G %d x %d" % (grid["n_a"], grid["n_b"]), []
        for which, variant in builds:
            g = d2pc.SectorsGround(variant=variant, **grid)
            out = ground_outputs(g.n_cells, 32)
            keep.append(g)
            outs.append(out)
            add(row, which, lambda g=g, out=out: g.process(level_cloud, level_n, gstep, counts=count, n_candidates=32, stream_ptr=s, **out))
        pairs.append((row, outs))
        cfg, tables, nc = g.cfg, outs[0], g.n_cells
        row, outs = "U %d x %d x %d" % (grid["n_a"], grid["n_b"], depth), []
        for which, variant in builds:
            ter = d2pc.SectorsTerrain(cfg, depth=depth, variant=variant)   # a window each
            out, status = ground_outputs(nc, 32), torch.zeros(4, dtype=torch.int32, device="cuda")
            keep.append(ter)
            outs.append(dict(out, status=status))
            add(row, which, lambda ter=ter, tables=tables, out=out, status=status: ter.update(gstep, tables["count"], tables["sum"], tables["sum2"],
                                                                                              n_candidates=32, status=status, stream_ptr=s, **out))
        pairs.append((row, outs))
        windows.append((row, depth, outs[0]["status"]))
    for _ in range(20):   # warm-up: code objects, and more updates than the deepest window holds
        for fn in arms[first:]:
            fn()
    torch.cuda.synchronize()
    for row, (new, old) in pairs[len(s_rows) + len(m_rows):]:
        assert same_bytes(new, old), row + ": the builds disagree"
    for row, depth, status in windows:
        took = int(status.cpu().numpy().view(np.uint32)[1])
        assert took == depth, "%s: %d slots took part" % (row, took)
    iters = int(min(max(a.iters, 30000.0 / timed(arms[0], 5)), 4000))   # (a sectors arm: no memory advances alone)
    t = dict(zip(labels, interleaved(arms, a.rounds, iters)))
    lines.append("# %d points, %.1f MB read by S; %d records of the level ground read by G; %d calls per timed window" % (npts, 16 * npts / 1e6, level_n, iters))
    lines += verdicts(t, [row for row, _ in pairs])
    for x in keep:
        if hasattr(x, "close"):
            x.close()
    for ln in lines:
        print(ln, flush=True)
    return lines


def memory(a):
    """The memory's update beside the sectors call it follows, all arms of all rows interleaved in one run."""
    prop = torch.cuda.get_device_properties(0)
    half_pi = float(np.float32(np.pi / 2))
    grids = [("72 x 1", dict()),
             ("60 x 30 elevation", dict(n_sectors=60, n_layers=30, u_min=-half_pi, u_max=half_pi, azimuth0=-np.pi / 60,
                                        layer_kind=d2pc.LAYERS_ELEVATION))]
    lines = ["# tools/sectors_bench.py --memory --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; every arm of this file interleaved round by round)" % (
                 prop.name, prop.multi_processor_count),
             "# S = d2pc_sectors_process_device alone (two launches; range, count, nearest); S0 = the same with every count 0;",
             "# M = d2pc_sectors_memory_update_device alone (one launch of one block; range, distance_cm, age; a 37-degree yaw, a",
             "# translation and dt 50 every call, max_age 2,000, a forward field of view as `covered`); SM = S then M on one stream.",
             "# us per call: median (min .. max) over the rounds.  No time was fixed in advance: M is read against S0 of its row"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    clouds, keep = [], []
    for name, n, w, h, mode, rig_case, holes in CASES[:2]:
        with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx:
            prod = Producer(ctx, n, w, h, rig_case, holes, gen)
            prod(s)
            torch.cuda.synchronize()
            ctx.check_async_error()
            npts = int(prod.offsets.cpu().numpy().view(np.uint32)[n]) if rig_case else int(prod.counts.cpu().numpy().view(np.uint32)[0])
            clouds.append((name, npts, prod.pts[:npts].clone()))
            prod.close()
    R = np.array([[np.cos(0.6458), 0.0, np.sin(0.6458)], [0.0, 1.0, 0.0], [-np.sin(0.6458), 0.0, np.cos(0.6458)]])   # about the optical y
    step = torch.from_numpy(d2pc.sectors_memory_step(R, [0.4, -0.1, 0.9], 50).view(np.int32).copy()).to("cuda")
    arms, labels, rows = [], [], []
    for cname, npts, cloud in clouds:
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        for gname, grid in grids:
            sec = d2pc.Sectors(**grid)
            mem = d2pc.SectorsMemory(sec.cfg, 2000)
            cov = torch.from_numpy(d2pc.sectors_memory_coverage(sec.cfg, [(0.0, 0.0, 1.5, 1.0, 0.05)])).to("cuda")
            so = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"),
                      count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"),
                      nearest=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
            mo = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"),
                      distance_cm=torch.empty(sec.n_cells, dtype=torch.int16, device="cuda"),
                      age=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
            so0 = {k: torch.empty_like(v) for k, v in so.items()}   # S0's own: M reads a full cloud's count / nearest from `so`
            keep.append((sec, mem, cov, so, so0, mo, zero))

            def sectors(sec=sec, cloud=cloud, npts=npts, so=so):
                sec.process(cloud, npts, stream_ptr=s, **so)

            def empty(sec=sec, cloud=cloud, npts=npts, so0=so0, zero=zero):
                sec.process(cloud, npts, counts=zero, stream_ptr=s, **so0)

            def update(mem=mem, cloud=cloud, npts=npts, so=so, mo=mo, cov=cov):
                mem.update(cloud, npts, so["count"], so["nearest"], step, covered=cov, stream_ptr=s, **mo)

            def both(sectors=sectors, update=update):
                sectors()
                update()

            row = "%s, %s" % (cname, gname)
            rows.append((row, npts, sec.n_cells))
            arms += [sectors, empty, update, both]
            labels += [row + " " + k for k in ("S", "S0", "M", "SM")]
    for fn in arms:   # warm-up: code objects
        fn()
    torch.cuda.synchronize()
    iters = int(min(max(a.iters, 30000.0 / timed(arms[3], 5)), 4000))
    t = dict(zip(labels, interleaved(arms, a.rounds, iters)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    lines.append("# %d calls per timed window" % iters)
    lines.append("%-62s %10s %6s %-30s %-30s %-30s %-30s %6s %8s" % ("cloud, grid", "points", "cells", "S", "S0", "M", "SM", "M/S0", "SM-S"))
    for row, npts, cells in rows:
        lines.append("%-62s %10d %6d %-30s %-30s %-30s %-30s %6.2f %8.1f" % (
            row, npts, cells, fmt(t[row + " S"]), fmt(t[row + " S0"]), fmt(t[row + " M"]), fmt(t[row + " SM"]),
            med[row + " M"] / med[row + " S0"], med[row + " SM"] - med[row + " S"]))
    for sec, mem, *_ in keep:
        mem.close()
        sec.close()
    for ln in lines:
        print(ln, flush=True)
    return lines


def steer(a):
    """The steer call beside the sectors call and the memory's update it follows, all arms of all rows interleaved in one run."""
    import sectors_steer_ref
    prop = torch.cuda.get_device_properties(0)
    lines = ["# tools/sectors_bench.py --steer%s --rounds %d --iters %d" % (" --parent " + a.parent if a.parent else "", a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; every arm of this file interleaved round by round)" % (
                 prop.name, prop.multi_processor_count),
             "# S0 = d2pc_sectors_process_device with every count 0 (the sectors' fixed part); M = d2pc_sectors_memory_update_device alone;",
             "# SM = the sectors call then M on one stream (as tools/sectors_bench.py --memory has them); T = d2pc_sectors_steer_device alone",
             "# (one launch of one block; radius 0.5, reach 8 sectors and 0 / 4 layers, clearance_cm, cost, 5 candidates and summary, from",
             "# the memory's distance_cm); T32 = the same with 32 candidates; SMT = SM then T on one stream.  us per call: median (min .. max)",
             "# over the rounds.  No time was fixed in advance: T is read against M and S0 of its row.  CPU = tests/sectors_steer_ref.py",
             "# (numpy, one core) on the same distance_cm, ms per call"]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    clouds, keep = [], []
    for name, n, w, h, mode, rig_case, holes in CASES[:2]:
        with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx:
            prod = Producer(ctx, n, w, h, rig_case, holes, gen)
            prod(s)
            torch.cuda.synchronize()
            ctx.check_async_error()
            npts = int(prod.offsets.cpu().numpy().view(np.uint32)[n]) if rig_case else int(prod.counts.cpu().numpy().view(np.uint32)[0])
            clouds.append((name, npts, prod.pts[:npts].clone()))
            prod.close()
    R = np.array([[np.cos(0.6458), 0.0, np.sin(0.6458)], [0.0, 1.0, 0.0], [-np.sin(0.6458), 0.0, np.cos(0.6458)]])   # about the optical y
    step = torch.from_numpy(d2pc.sectors_memory_step(R, [0.4, -0.1, 0.9], 50).view(np.int32).copy()).to("cuda")
    arms, labels, rows, versus = [], [], [], []
    for cname, npts, cloud in clouds:
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        for gname, grid, reach in STEER_GRIDS:
            sec = d2pc.Sectors(**grid)
            mem = d2pc.SectorsMemory(sec.cfg, 2000)
            st = d2pc.SectorsSteer(sec.cfg, **reach)
            goal = torch.from_numpy(d2pc.sectors_steer_step(sec.cfg.n_sectors // 3, sec.cfg.n_layers // 2, 1, sec.cfg.n_layers // 2)
                                    .view(np.int32).copy()).to("cuda")
            cov = torch.from_numpy(d2pc.sectors_memory_coverage(sec.cfg, [(0.0, 0.0, 1.5, 1.0, 0.05)])).to("cuda")
            so = dict(count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"),
                      nearest=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
            so0 = {k: torch.empty_like(v) for k, v in so.items()}   # S0's own: M reads a full cloud's count / nearest from `so`
            mo = dict(distance_cm=torch.empty(sec.n_cells, dtype=torch.int16, device="cuda"))
            to = steer_outputs(sec.n_cells, 32)
            keep.append((sec, mem, st, goal, cov, so, so0, mo, to, zero))

            def sectors(sec=sec, cloud=cloud, npts=npts, so=so):
                sec.process(cloud, npts, stream_ptr=s, **so)

            def empty(sec=sec, cloud=cloud, npts=npts, so0=so0, zero=zero):
                sec.process(cloud, npts, counts=zero, stream_ptr=s, **so0)

            def update(mem=mem, cloud=cloud, npts=npts, so=so, mo=mo, cov=cov):
                mem.update(cloud, npts, so["count"], so["nearest"], step, covered=cov, stream_ptr=s, **mo)

            def turn(st=st, mo=mo, to=to, goal=goal, k=5):
                st.steer(mo["distance_cm"], goal, n_candidates=k, stream_ptr=s, **to)

            def turn32(turn=turn):
                turn(k=32)

            def both(sectors=sectors, update=update):
                sectors()
                update()

            def three(both=both, turn=turn):
                both()
                turn()

            row = "%s, %s" % (cname, gname)
            rows.append((row, npts, sec, st, mo, goal))
            arms += [empty, update, both, turn, turn32, three]
            labels += [row + " " + k for k in ("S0", "M", "SM", "T", "T32", "SMT")]
            if a.parent:   # the other build's steer on the same input, with outputs of its own
                other = d2pc.SectorsSteer(sec.cfg, variant=a.parent, **reach)
                oo = {k: torch.empty_like(v) for k, v in to.items()}
                keep.append((None, None, other, oo))
                arms += [lambda other=other, mo=mo, oo=oo, goal=goal: other.steer(mo["distance_cm"], goal, n_candidates=5, stream_ptr=s, **oo),
                         lambda other=other, mo=mo, oo=oo, goal=goal: other.steer(mo["distance_cm"], goal, n_candidates=32, stream_ptr=s, **oo)]
                labels += [row + " T " + a.parent, row + " T32 " + a.parent]
                versus.append((row, to, oo, turn32, arms[-1]))
    for _ in range(3):   # warm-up: code objects; three updates, so that the memories hold what left the field of view
        for fn in arms:
            fn()
    torch.cuda.synchronize()
    for row, to, oo, mine, theirs in versus:   # 32 candidates of both builds from the same distance_cm
        mine()
        theirs()
        torch.cuda.synchronize()
        assert all(torch.equal(to[k], oo[k]) for k in to), row + ": the builds disagree"
    iters = int(min(max(a.iters, 30000.0 / timed(arms[2], 5)), 4000))
    t = dict(zip(labels, interleaved(arms, a.rounds, iters)))
    med = {k: float(np.median(v)) for k, v in t.items()}
    lines.append("# %d calls per timed window" % iters)
    lines.append("%-62s %10s %6s %6s %-30s %-30s %-30s %-30s %-30s %-30s %6s %6s %8s %7s" % (
        "cloud, grid", "points", "cells", "free", "S0", "M", "SM", "T", "T32", "SMT", "T/M", "T/S0", "SMT-SM", "CPU ms"))
    for row, npts, sec, st, mo, goal in rows:
        torch.cuda.synchronize()
        dcm = mo["distance_cm"].cpu().numpy().view(np.uint16)
        ref = sectors_steer_ref.SectorsSteerRef(sec.cfg, st.scfg, *d2pc.sectors_steer_reach(sec.cfg, st.scfg))
        t0 = time.perf_counter()
        want = ref.steer(dcm, goal.cpu().numpy().view(np.uint32), None, 5)
        cpu = (time.perf_counter() - t0) * 1e3
        lines.append("%-62s %10d %6d %6d %-30s %-30s %-30s %-30s %-30s %-30s %6.2f %6.2f %8.1f %7.2f" % (
            row, npts, sec.n_cells, int(want["summary"][0]), fmt(t[row + " S0"]), fmt(t[row + " M"]), fmt(t[row + " SM"]), fmt(t[row + " T"]),
            fmt(t[row + " T32"]), fmt(t[row + " SMT"]), med[row + " T"] / med[row + " M"], med[row + " T"] / med[row + " S0"],
            med[row + " SMT"] - med[row + " SM"], cpu))
    if a.parent:
        lines.append("# the steer of libd2pc_sectors_%s.so (`make sectors SNAME=%s` of other sources) on the same input in the same run; the two builds'" % (a.parent, a.parent))
        lines.append("# outputs (32 candidates) were compared bit for bit before the timing")
        lines.append("%-62s %-30s %-30s %-30s %-30s %8s %8s" % ("cloud, grid", "T", "T " + a.parent, "T32", "T32 " + a.parent, "T ratio", "T32 ratio"))
        for row, *_ in rows:
            lines.append("%-62s %-30s %-30s %-30s %-30s %8.2f %8.2f" % (
                row, fmt(t[row + " T"]), fmt(t[row + " T " + a.parent]), fmt(t[row + " T32"]), fmt(t[row + " T32 " + a.parent]),
                med[row + " T " + a.parent] / med[row + " T"], med[row + " T32 " + a.parent] / med[row + " T32"]))
    for sec, mem, st, *_ in keep:
        st.close()
        if mem is not None:
            mem.close()
            sec.close()
    for ln in lines:
        print(ln, flush=True)
    return lines


def ground(a):
    """The landing grid beside the sectors call on the same cloud."""
    prop = torch.cuda.get_device_properties(0)
    size = os.path.getsize(d2pc.sectors_library_path())
    lines = ["# tools/sectors_bench.py --ground --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; arms interleaved round by round); libd2pc_sectors.so is %d bytes" % (
                 prop.name, prop.multi_processor_count, size),
             "# the frames are a level ground 5.4 m below a camera that looks straight down (disparity 94 .. 98, 30 % holes), the pose in the step is",
             "# that nadir pose: a row of 64 neighbouring records spans about 0.5 m.  The grid is 8 m x 8 m under the camera: 16 x 16 cells of 0.5 m or",
             "# 64 x 64 of 0.125 m, quantum 0.002, all nine outputs with 5 candidates, max_points = the cloud's capacity; a cell is flat up to a standard",
             "# deviation of 0.15 m (the quantised depths spread by 0.08 m) and max_step_q is 100, so the one-camera frame makes sites and all 5 candidate rounds run (the line under a row says how many).  Of the rig's merged cloud only",
             "# the camera that looks down and its neighbours reach the grid; the other records are gated out after the transform.",
             "# G = d2pc_sectors_ground_process_device alone (three launches); G0 = the same call with a count of 0: the fixed part;",
             "# C = d2pc_membench_copy moving the bytes G reads (16 B per record); S / S0 = the 72 x 1 sectors call on the same cloud / with a count of 0;",
             "# us per call: median (min .. max) over the rounds",
             "%-52s %9s %6s %-30s %-30s %-30s %-30s %-30s %5s %5s %6s" % ("cloud, grid", "records", "blocks", "G", "G0", "C", "S", "S0", "G/C", "G/S", "G0/S0")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    for name, n, w, h, mode, rig_case, holes in CASES[:2]:
        with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx, d2pc.Sectors() as sec:
            prod = Producer(ctx, n, w, h, rig_case, holes, gen)
            npts, ordered, corner = level_ground(ctx, prod, gen, s)
            step = ground_step(corner)
            shuffled = ordered[torch.randperm(npts, generator=gen, device="cuda")].contiguous()
            count = torch.tensor([npts], dtype=torch.int32, device="cuda")
            zero = torch.zeros(1, dtype=torch.int32, device="cuda")
            half = max(16 * npts // 2 // 16 * 16, 16)
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            s_out = dict(range=torch.empty(sec.n_cells, dtype=torch.float32, device="cuda"), count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"),
                         nearest=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"), distance_cm=torch.empty(sec.n_cells, dtype=torch.int16, device="cuda"))
            for grid, _ in GROUND_GRIDS:
                grid = ground_grid(grid, prod)
                session = d2pc.SectorsGround(**grid)
                out = ground_outputs(session.n_cells, 5)
                for label, cloud in (("producer order", ordered), ("shuffled", shuffled)):
                    def call(g, o, c):
                        return lambda: g.process(cloud, npts, step, counts=c, n_candidates=5, stream_ptr=s, **o)

                    arms = [call(session, out, count), call(session, out, zero),
                            lambda: ctx.membench_copy(src.data_ptr(), dst.data_ptr(), half, s),
                            lambda: sec.process(cloud, npts, counts=count, stream_ptr=s, **s_out),
                            lambda: sec.process(cloud, npts, counts=zero, stream_ptr=s, **s_out)]
                    for fn in arms[:1] + arms[2:]:
                        fn()
                    torch.cuda.synchronize()
                    summary = tuple(int(v) for v in out["summary"].cpu().numpy().view(np.uint32)[:3])
                    assert 0 < summary[0] <= npts, "no record reached the grid"
                    assert rig_case or summary[2] >= 5, "the one-camera frame makes fewer sites than candidates"
                    iters = int(min(max(a.iters, 30000.0 / timed(arms[0], 5)), 4000))
                    t = interleaved(arms, a.rounds, iters)
                    ctx.check_async_error()
                    m = [float(np.median(x)) for x in t]
                    lines.append("%-52s %9d %6d %-30s %-30s %-30s %-30s %-30s %5.2f %5.2f %6.2f" % (
                        "%s, %d x %d, %s" % (name[:14].strip(), grid["n_a"], grid["n_b"], label), npts, min(session.blocks, (npts + 1023) // 1024),
                        fmt(t[0]), fmt(t[1]), fmt(t[2]), fmt(t[3]), fmt(t[4]), m[0] / m[2], m[0] / m[3], m[1] / m[4]))
                    lines.append("#   %d of the records took part, %d flat cells, %d sites" % summary)
                    print(lines[-2], flush=True)
                session.close()
            prod.close()
        del prod, ordered, shuffled, src, dst
        torch.cuda.empty_cache()
    return lines


SLOPE_GRIDS = [dict(n_a=16, n_b=16, cell_size=0.5), dict(n_a=46, n_b=46, cell_size=0.125)]


def slope_outputs(nc, k):
    return dict(count=torch.empty(nc, dtype=torch.int32, device="cuda"), sum=torch.empty(nc, dtype=torch.int64, device="cuda"),
                sum2=torch.empty(nc, dtype=torch.int64, device="cuda"), moments=torch.empty(7 * nc, dtype=torch.int64, device="cuda"),
                slope_a=torch.empty(nc, dtype=torch.float32, device="cuda"), slope_b=torch.empty(nc, dtype=torch.float32, device="cuda"),
                level_q=torch.empty(nc, dtype=torch.int32, device="cuda"), resid_q2=torch.empty(nc, dtype=torch.int32, device="cuda"),
                flat=torch.empty(nc, dtype=torch.uint8, device="cuda"), site=torch.empty(nc, dtype=torch.uint8, device="cuda"),
                candidates=torch.empty(k, dtype=torch.int64, device="cuda"), summary=torch.empty(4, dtype=torch.int32, device="cuda"))


def slope(a):
    """The plane fit per cell beside the ground call of the same configuration on the same cloud."""
    prop = torch.cuda.get_device_properties(0)
    size = os.path.getsize(d2pc.sectors_library_path())
    lines = ["# tools/sectors_bench.py --slope --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; arms interleaved round by round); libd2pc_sectors.so is %d bytes" % (
                 prop.name, prop.multi_processor_count, size),
             "# the cloud is tools/sectors_bench.py --ground's: a level ground 5.4 m below a camera that looks straight down (30 % holes), the nadir pose in",
             "# the step.  The grid lies under the camera: 16 x 16 cells of 0.5 m or 46 x 46 of 0.125 m (the largest square table of one block's LDS: 160,816",
             "# bytes, one block a CU), quantum 0.002, sub 8, max_slope tan 15 deg, max_points = the cloud's capacity, every output with 5 candidates.",
             "# L = d2pc_sectors_slope_process_device alone (three launches, all twelve outputs); L0 = the same call with a count of 0: the fixed part (tables",
             "# initialised, slabs of 76 bytes a cell stored and merged, the fit, the sites); G / G0 = d2pc_sectors_ground_process_device of the same",
             "# configuration, likewise (nine outputs, slabs of 20 bytes a cell); C = d2pc_membench_copy moving the bytes L and G read (16 B per record).",
             "# slabs = L0 - G0: what the larger tables cost with no record read; adds = (L - L0) - (G - G0): what ten LDS adds a record cost over three.",
             "# us per call: median (min .. max) over the rounds.  No time was fixed in advance",
             "%-52s %9s %7s %-30s %-30s %-30s %-30s %-30s %5s %5s %6s %7s %7s" % ("cloud, grid", "records", "blocks", "L", "L0", "G", "G0", "C", "L/G", "L/C", "L0/G0",
                                                                            "slabs", "adds")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    for name, n, w, h, mode, rig_case, holes in CASES[:2]:
        with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx:
            prod = Producer(ctx, n, w, h, rig_case, holes, gen)
            npts, ordered, corner = level_ground(ctx, prod, gen, s)
            step = ground_step(corner)
            shuffled = ordered[torch.randperm(npts, generator=gen, device="cuda")].contiguous()
            count = torch.tensor([npts], dtype=torch.int32, device="cuda")
            zero = torch.zeros(1, dtype=torch.int32, device="cuda")
            half = max(16 * npts // 2 // 16 * 16, 16)
            src = torch.empty(half, dtype=torch.uint8, device="cuda")
            dst = torch.empty(half, dtype=torch.uint8, device="cuda")
            for grid in SLOPE_GRIDS:
                grid = ground_grid(grid, prod)
                gnd = d2pc.SectorsGround(**grid)
                slp = d2pc.SectorsSlope(gnd.cfg)
                g_out, l_out = ground_outputs(gnd.n_cells, 5), slope_outputs(slp.n_cells, 5)
                for label, cloud in (("producer order", ordered), ("shuffled", shuffled)):
                    def call(x, o, c):
                        return lambda: x.process(cloud, npts, step, counts=c, n_candidates=5, stream_ptr=s, **o)

                    arms = [call(slp, l_out, count), call(slp, l_out, zero), call(gnd, g_out, count), call(gnd, g_out, zero),
                            lambda: ctx.membench_copy(src.data_ptr(), dst.data_ptr(), half, s)]
                    for fn in (arms[0], arms[2], arms[4]):
                        fn()
                    torch.cuda.synchronize()
                    ls = tuple(int(v) for v in l_out["summary"].cpu().numpy().view(np.uint32))
                    gs = tuple(int(v) for v in g_out["summary"].cpu().numpy().view(np.uint32))
                    assert 0 < ls[0] <= npts and ls[0] == gs[0], "the two calls took different records"
                    assert torch.equal(l_out["count"], g_out["count"]) and torch.equal(l_out["sum2"], g_out["sum2"])
                    iters = int(min(max(a.iters, 30000.0 / timed(arms[0], 5)), 4000))
                    t = interleaved(arms, a.rounds, iters)
                    ctx.check_async_error()
                    m = [float(np.median(x)) for x in t]
                    lines.append("%-52s %9d %7s %-30s %-30s %-30s %-30s %-30s %5.2f %5.2f %6.2f %7.1f %7.1f" % (
                        "%s, %d x %d, %s" % (name[:14].strip(), grid["n_a"], grid["n_b"], label), npts,
                        "%d/%d" % (min(slp.blocks, (npts + 1023) // 1024), min(gnd.blocks, (npts + 1023) // 1024)),
                        fmt(t[0]), fmt(t[1]), fmt(t[2]), fmt(t[3]), fmt(t[4]), m[0] / m[2], m[0] / m[4], m[1] / m[3], m[1] - m[3], (m[0] - m[1]) - (m[2] - m[3])))
                    lines.append("#   %d of the records took part; slope: %d flat cells, %d sites, %d fitted; ground: %d flat cells, %d sites" % (
                        ls[0], ls[1], ls[2], ls[3], gs[1], gs[2]))
                    print(lines[-2], flush=True)
                slp.close()
                gnd.close()
            prod.close()
        del prod, ordered, shuffled, src, dst
        torch.cuda.empty_cache()
    return lines


def terrain(a):
    """The terrain's update alone beside the ground call that feeds it and the steer call, on one cloud, in one run."""
    prop = torch.cuda.get_device_properties(0)
    size = os.path.getsize(d2pc.sectors_library_path())
    lines = ["# tools/sectors_bench.py --terrain --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; every arm of this file interleaved round by round); libd2pc_sectors.so is %d bytes" % (
                 prop.name, prop.multi_processor_count, size),
             "# the cloud is tools/sectors_bench.py --ground's one-camera frame (a level ground under a nadir camera, 30 % holes) in producer order; the",
             "# grid is 8 m x 8 m under the camera, all nine outputs with 5 candidates and status.",
             "# G = d2pc_sectors_ground_process_device alone (three launches); G0 = the same call with a count of 0: the ground's fixed part;",
             "# T all = d2pc_sectors_terrain_update_device alone (ONE launch of one block) on G's count / sum / sum2 with the corner held, so every slot",
             "# of the window takes part (depth - 1 stored tables are read whole); T none = the same with a NaN h0 in the step: the frame is anchored and",
             "# stored, no stored table matches it, the window is the frame alone; ST = d2pc_sectors_steer_device alone (72 x 1, reach 8, 5 candidates) on",
             "# the distance_cm the sectors call and the memory's update made from the same cloud.  us per call: median (min .. max) over the rounds.",
             "# No time was fixed in advance: T is read against G0 and G of its row",
             "%-34s %9s %5s %-30s %-30s %-30s %-30s %-30s %8s %8s %8s" % ("cloud, grid x depth", "records", "took", "G", "G0", "T all", "T none", "ST",
                                                                    "Tall/G0", "Tall/G", "Tnone/G0")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    name, n, w, h, mode, rig_case, holes = CASES[0]
    with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx, d2pc.Sectors() as sec:
        prod = Producer(ctx, n, w, h, rig_case, holes, gen)
        npts, cloud, corner = level_ground(ctx, prod, gen, s)
        step = ground_step(corner)
        lone = torch.from_numpy(d2pc.sectors_ground_step(NADIR, [0.0, 0.0, 10.0], corner[:2] + [np.nan], 8, 8).view(np.int32).copy()).to("cuda")
        count = torch.tensor([npts], dtype=torch.int32, device="cuda")
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        # the steer's input: the sectors call and one update of the memory on the same cloud
        mem = d2pc.SectorsMemory(sec.cfg, 2000)
        st = d2pc.SectorsSteer(sec.cfg, max_reach_sectors=8, max_reach_layers=0)
        so = dict(count=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"), nearest=torch.empty(sec.n_cells, dtype=torch.int32, device="cuda"))
        mo = dict(distance_cm=torch.empty(sec.n_cells, dtype=torch.int16, device="cuda"))
        to = steer_outputs(sec.n_cells, 5)
        mstep = torch.from_numpy(d2pc.sectors_memory_step(np.eye(3), [0.0, 0.0, 0.0], 50).view(np.int32).copy()).to("cuda")
        goal = torch.from_numpy(d2pc.sectors_steer_step(sec.cfg.n_sectors // 3, 0, 1, 0).view(np.int32).copy()).to("cuda")
        sec.process(cloud, npts, stream_ptr=s, **so)
        mem.update(cloud, npts, so["count"], so["nearest"], mstep, stream_ptr=s, **mo)
        rows, arms, keep = [], [lambda: st.steer(mo["distance_cm"], goal, n_candidates=5, stream_ptr=s, **to)], []
        for grid, depth in GROUND_GRIDS:
            g = d2pc.SectorsGround(**ground_grid(grid, prod))

            def outputs(nc=g.n_cells):
                return ground_outputs(nc, 5)

            go, g0, t_all, t_none = outputs(), outputs(), outputs(), outputs()
            status = [torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(2)]
            ter = [d2pc.SectorsTerrain(g.cfg, depth=depth) for _ in range(2)]   # a window each: the two arms do not disturb each other
            keep.append((g, ter, go, g0, t_all, t_none, status))
            g.process(cloud, npts, step, counts=count, n_candidates=5, stream_ptr=s, **go)
            arms += [lambda g=g, go=go: g.process(cloud, npts, step, counts=count, n_candidates=5, stream_ptr=s, **go),
                     lambda g=g, g0=g0: g.process(cloud, npts, step, counts=zero, n_candidates=5, stream_ptr=s, **g0),
                     lambda t=ter[0], go=go, o=t_all, st_=status[0]: t.update(step, go["count"], go["sum"], go["sum2"], n_candidates=5, status=st_, stream_ptr=s, **o),
                     lambda t=ter[1], go=go, o=t_none, st_=status[1]: t.update(lone, go["count"], go["sum"], go["sum2"], n_candidates=5, status=st_, stream_ptr=s, **o)]
            rows.append(("%s, %d x %d x %d" % (name[:14].strip(), grid["n_a"], grid["n_b"], depth), depth, status))
        for _ in range(20):   # warm-up: code objects, and more updates than the deepest window holds
            for fn in arms:
                fn()
        torch.cuda.synchronize()
        ctx.check_async_error()
        for row, depth, status in rows:
            took = [int(x.cpu().numpy().view(np.uint32)[1]) for x in status]
            assert took == [depth, 1], "%s: %s slots took part" % (row, took)
        iters = int(min(max(a.iters, 30000.0 / timed(arms[1], 5)), 4000))
        t = interleaved(arms, a.rounds, iters)
        ctx.check_async_error()
        lines.insert(-1, "# %d calls per timed window" % iters)
        for k, (row, depth, status) in enumerate(rows):
            G, G0, Ta, Tn = t[1 + 4 * k:5 + 4 * k]
            m = [float(np.median(x)) for x in (G, G0, Ta, Tn)]
            lines.append("%-34s %9d %5d %-30s %-30s %-30s %-30s %-30s %8.2f %8.2f %8.2f" % (
                row, npts, depth, fmt(G), fmt(G0), fmt(Ta), fmt(Tn), fmt(t[0]), m[2] / m[1], m[2] / m[0], m[3] / m[1]))
        for g, ter, *_ in keep:
            for x in ter:
                x.close()
            g.close()
        st.close()
        mem.close()
        prod.close()
    for ln in lines:
        print(ln, flush=True)
    return lines


RELIEF_GRIDS = [(dict(n_a=16, n_b=16, cell_size=0.5), 8), (dict(n_a=46, n_b=46, cell_size=0.125), 16)]   # (grid, depth)


def relief(a):
    """The relief's update alone beside the slope call that feeds it, the terrain's update at the same grid and depth and a
    copy of the bytes the update reads, on one cloud, in one run."""
    prop = torch.cuda.get_device_properties(0)
    size = os.path.getsize(d2pc.sectors_library_path())
    lines = ["# tools/sectors_bench.py --relief --rounds %d --iters %d" % (a.rounds, a.iters),
             "# device draw: %s, %d CUs (one device, one process, ONE run; every arm of this file interleaved round by round); libd2pc_sectors.so is %d bytes" % (
                 prop.name, prop.multi_processor_count, size),
             "# the cloud is tools/sectors_bench.py --ground's one-camera frame (a level ground under a nadir camera, 30 % holes) in producer order; the",
             "# grid lies under the camera, quantum 0.002, sub 8, max_slope tan 15 deg, every output with 5 candidates (and status).",
             "# L = d2pc_sectors_slope_process_device alone (three launches); L0 = the same call with a count of 0: the slope's fixed part;",
             "# R all = d2pc_sectors_relief_update_device alone (TWO launches: the window and the fit in n_cells / 16 blocks, then one block) on L's count /",
             "# sum / sum2 / moments with the corner held, so every slot of the window takes part (depth - 1 stored tables of 76 bytes a cell are read whole);",
             "# R none = the same with a NaN h0 in the step: the frame is anchored and stored, no stored table matches it, the window is the frame alone;",
             "# T all = d2pc_sectors_terrain_update_device (ONE launch of one block, 20 bytes a cell) of the same grid and depth on L's count / sum / sum2,",
             "# every slot taking part; C = d2pc_membench_copy moving `read` bytes = depth x 76 x n_cells, what R all reads of tables (the frame's and the",
             "# stored).  GB/s = the bytes of the depth - 1 stored tables over the WHOLE of R all, both launches' fixed parts included: a lower bound on the",
             "# window launch's rate (R all - R none, the column before it, can lie inside the run's spread).  us per call: median (min .. max) over the rounds.",
             "# No time was fixed in advance",
             "%-34s %9s %5s %9s %-30s %-30s %-30s %-30s %-30s %-30s %7s %7s %7s %7s %7s %7s" % (
                 "cloud, grid x depth", "records", "took", "read", "R all", "R none", "L", "L0", "T all", "C", "Rall/C", "Rall/L0", "Rall/T", "Rnon/L0", "Ra-Rn", "GB/s")]
    gen = torch.Generator(device="cuda").manual_seed(1)
    s = torch.cuda.current_stream().cuda_stream
    name, n, w, h, mode, rig_case, holes = CASES[0]
    with d2pc.Context(q=d2pc.make_q(), border=BORDER, mode=mode) as ctx:
        prod = Producer(ctx, n, w, h, rig_case, holes, gen)
        npts, cloud, corner = level_ground(ctx, prod, gen, s)
        step = ground_step(corner)
        lone = torch.from_numpy(d2pc.sectors_ground_step(NADIR, [0.0, 0.0, 10.0], corner[:2] + [np.nan], 8, 8).view(np.int32).copy()).to("cuda")
        count = torch.tensor([npts], dtype=torch.int32, device="cuda")
        zero = torch.zeros(1, dtype=torch.int32, device="cuda")
        rows, arms, keep = [], [], []
        for grid, depth in RELIEF_GRIDS:
            slp = d2pc.SectorsSlope(d2pc.sectors_ground_config_init(**ground_grid(grid, prod)))
            nc = slp.n_cells
            lo, l0, r_all, r_none = [slope_outputs(nc, 5) for _ in range(4)]
            t_all = ground_outputs(nc, 5)
            status = [torch.zeros(4, dtype=torch.int32, device="cuda") for _ in range(3)]
            rel = [d2pc.SectorsRelief(slp.cfg, slp.scfg, depth=depth) for _ in range(2)]   # a window each: the two arms do not disturb each other
            ter = d2pc.SectorsTerrain(slp.cfg, depth=depth)
            wide = os.path.exists(d2pc.sectors_library_path("relief64"))   # `make sectors SNAME=relief64 SDEFS=-DD2PC_SECTORS_RELIEF_CELLS=64`
            if wide:
                rel.append(d2pc.SectorsRelief(slp.cfg, slp.scfg, depth=depth, variant="relief64"))
                r_wide, status = slope_outputs(nc, 5), status + [torch.zeros(4, dtype=torch.int32, device="cuda")]
            read = depth * 76 * nc
            src, dst = torch.empty(read, dtype=torch.uint8, device="cuda"), torch.empty(read, dtype=torch.uint8, device="cuda")
            keep.append((slp, rel, ter, lo, l0, r_all, r_none, t_all, status, src, dst))
            slp.process(cloud, npts, step, counts=count, n_candidates=5, stream_ptr=s, **lo)

            def update(r, st_step, o, st_, lo=lo):
                return lambda: r.update(st_step, lo["count"], lo["sum"], lo["sum2"], lo["moments"], n_candidates=5, status=st_, stream_ptr=s, **o)

            def update_terrain(lo=lo, t_all=t_all, st_=status[2], ter=ter):
                ter.update(step, lo["count"], lo["sum"], lo["sum2"], n_candidates=5, status=st_, stream_ptr=s, **t_all)

            arms += [update(rel[0], step, r_all, status[0]), update(rel[1], lone, r_none, status[1]),
                     lambda slp=slp, lo=lo: slp.process(cloud, npts, step, counts=count, n_candidates=5, stream_ptr=s, **lo),
                     lambda slp=slp, l0=l0: slp.process(cloud, npts, step, counts=zero, n_candidates=5, stream_ptr=s, **l0),
                     update_terrain,
                     lambda src=src, dst=dst, read=read: ctx.membench_copy(src.data_ptr(), dst.data_ptr(), read, s),
                     update(rel[2], step, r_wide, status[3]) if wide else (lambda: None)]
            rows.append(("%s, %d x %d x %d" % (name[:14].strip(), grid["n_a"], grid["n_b"], depth), depth, read, nc, status, lo, r_all))
            if wide:
                keep.append(r_wide)
        for _ in range(20):   # warm-up: code objects, and more updates than the deepest window holds
            for fn in arms:
                fn()
        torch.cuda.synchronize()
        ctx.check_async_error()
        for row, depth, read, nc, status, lo, r_all in rows:
            took = [int(x.cpu().numpy().view(np.uint32)[1]) for x in status]
            assert took == [depth, 1, depth] + [depth] * (len(status) - 3), "%s: %s slots took part" % (row, took)
            assert torch.equal(r_all["count"], lo["count"] * depth) and torch.equal(r_all["moments"], lo["moments"] * depth), "the window is not depth frames"
        iters = int(min(max(a.iters, 30000.0 / timed(arms[3], 5)), 4000))
        t = interleaved(arms, a.rounds, iters)
        ctx.check_async_error()
        lines.insert(-1, "# %d calls per timed window" % iters)
        for k, (row, depth, read, nc, status, lo, r_all) in enumerate(rows):
            Ra, Rn, L, L0, Ta, C, Rw = t[7 * k:7 * k + 7]
            m = [float(np.median(x)) for x in (Ra, Rn, L, L0, Ta, C)]
            stored = (depth - 1) * 76 * nc
            lines.append("%-34s %9d %5d %9d %-30s %-30s %-30s %-30s %-30s %-30s %7.2f %7.2f %7.2f %7.2f %7.1f %7.1f" % (
                row, npts, depth, read, fmt(Ra), fmt(Rn), fmt(L), fmt(L0), fmt(Ta), fmt(C), m[0] / m[5], m[0] / m[3], m[0] / m[4], m[1] / m[3],
                m[0] - m[1], stored / m[0] / 1000.0))
            fs = tuple(int(v) for v in r_all["summary"].cpu().numpy().view(np.uint32))
            lines.append("#   the window of %d frames: %d points, %d flat cells, %d sites, %d fitted of %d cells; %d blocks" % (depth, fs[0], fs[1], fs[2], fs[3], nc,
                                                                                                                      (nc + 15) // 16))
            if len(status) > 3:
                lines.append("#   R all of the 64 cells x 4 slices build (libd2pc_sectors_relief64.so, %d blocks, four list entries a lane): %s" % ((nc + 63) // 64, fmt(Rw)))
        for slp, rel, ter, *_ in [x for x in keep if isinstance(x, tuple)]:
            for x in rel:
                x.close()
            ter.close()
            slp.close()
        prod.close()
    for ln in lines:
        print(ln, flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--only", type=int, default=None, help="one case only, by its index (a profiler run)")
    ap.add_argument("--ab", action="store_true", help="the A/B of the in-wave reduction instead of the cost table")
    ap.add_argument("--elevation", action="store_true", help="elevation layers beside height layers instead of the cost table")
    ap.add_argument("--memory", action="store_true", help="the memory's update beside the sectors call instead of the cost table")
    ap.add_argument("--steer", action="store_true", help="the steer call beside the sectors call and the memory's update instead of the cost table")
    ap.add_argument("--ground", action="store_true", help="the landing grid beside the sectors call instead of the cost table")
    ap.add_argument("--terrain", action="store_true", help="the terrain's update beside the ground call and the steer call instead of the cost table")
    ap.add_argument("--slope", action="store_true", help="the plane fit per cell beside the ground call instead of the cost table")
    ap.add_argument("--relief", action="store_true", help="the relief's update beside the slope call, the terrain's update and a copy instead of the cost table")
    ap.add_argument("--parent", default=None, help="libd2pc_sectors_<PARENT>.so, an earlier build: with --elevation beside the height rows; "
                    "alone, the table of this build against it (S, M, T, T32, G and the terrain's update)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.parent and (a.memory or a.ab or a.ground or a.terrain or a.slope or a.relief):
        ap.error("--parent goes with --elevation or --steer or stands alone (its own table holds the memory's rows)")
    versus = bool(a.parent) and not (a.memory or a.elevation or a.ab or a.steer)
    if a.ground or a.terrain or a.slope or a.relief:
        lines = relief(a) if a.relief else slope(a) if a.slope else terrain(a) if a.terrain else ground(a)
        out = a.out or os.path.join(ROOT, "profiles", "sectors_relief_bench.txt" if a.relief else "sectors_slope_bench.txt" if a.slope else "sectors_terrain_bench.txt" if a.terrain else "sectors_ground_bench.txt")
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
        print("wrote", out)
        return
    out = a.out or os.path.join(ROOT, "profiles", "sectors_steer_bench.txt" if a.steer else "sectors_memory_bench.txt" if a.memory else "sectors_elevation_bench.txt" if a.elevation else "sectors_ab.txt" if a.ab else "sectors_refactor_bench.txt" if versus else "sectors_bench.txt")
    lines = steer(a) if a.steer else memory(a) if a.memory else elevation(a) if a.elevation else ab(a) if a.ab else parent(a) if versus else bench(a)
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
