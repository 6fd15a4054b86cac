"""csrc/d2pc_route.hpp -- the launch plans behind enqueue and d2pc_process_mono_device -- without a GPU:
tests/cpp/route_plan_main.cpp, built with plain g++ under ASan + UBSan (the header includes nothing of HIP), checks its
own invariants over a grid of its own and answers queries, whose plans are compared here with tests/route_model.py --
the model the GPU tests hold against d2pc_compact_stats.  The grid sits at the seams, not at the workload sizes:

  COMPACT   cu {8, 64, 256, 304} x frames {1, 2, 3, 4, 5, 16, cap + 1} (cap = 4 cu) x compact_algo 0..3 x force_algo 0..3 x
            resident_pxt {0, 32, 64} x onepass_form {0, 2} x captured {0, 1} x ROI sizes 256 r k + {-1, 0, 1} for r in
            {8, 32, 64}, k in {1, cap // n, cap // n + 1, 1024, 1025}, and the ROI sizes of BIG_SEAM_TILES tiles: n x tiles
            is 20,480 exactly for n = 4 at 5,120 tiles and 20,481 for n = 3 at 6,827; 20,479 has no divisor 3 or 4, so the
            seam's lower side is 4 x 5,119 = 20,476 and 3 x 6,826 = 20,478 (every frame count meets every size)
  callback  cu as above x callback_pipe_blocks_per_cu 1..3 x fused form {1, 2} x tiles_x {1, 2, 5, 127, 128} x tiles_y
            {1, 3, 130} x frames {1, nfc - 1, nfc, nfc + 1, 2 nfc - 1, 2 nfc, 2 nfc + 1}
  overlap   callback_chunks {0, 1, 2, 4} x frames {1, 2, 16} x frame sizes either side of 16 Mi pixels per chunk x the flags
  PARITY    the 96,000,000-pixel seam of the 8- / 16-bit launches"""
import itertools
import os
import subprocess

import pytest

import route_model as rm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = (8, 64, 256, 304)
BIG_SEAM_TILES = (5119, 5120, 5121, 6826, 6827)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("route") / "route_plan"
    src = os.path.join(ROOT, "tests", "cpp", "route_plan_main.cpp")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-omit-frame-pointer", "-o", str(out), src], check=True, capture_output=True, timeout=180)
    return str(out)


def run(exe, args=(), text=""):
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    p = subprocess.run([exe, *args], input=text, capture_output=True, text=True, timeout=300, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    return p.stdout


def test_the_header_compiles_without_hip_and_keeps_its_invariants(exe):
    out = run(exe, ["check"])
    assert "route check ok" in out, out
    compact, callback = (int(out.split()[i]) for i in (3, 6))
    assert compact > 10_000_000 and callback > 100_000, out


def roi_sizes(cap, n):
    out = {256 * r * k + d for r in (8, 32, 64) for k in (1, cap // n, cap // n + 1, 1024, 1025) for d in (-1, 0, 1)}
    out |= {2048 * t for t in BIG_SEAM_TILES}
    return sorted(x for x in out if x >= 1)


def compact_queries():
    for cu in CUS:
        cap = 4 * cu
        for n in (1, 2, 3, 4, 5, 16, cap + 1):
            sizes = roi_sizes(cap, n)
            for algo, force, rpxt, form, captured in itertools.product(range(4), range(4), (0, 32, 64), (0, 2), (0, 1)):
                for roi_n in sizes:
                    yield cu, algo, force, rpxt, form, captured, n, roi_n


def test_compact_plans_equal_the_model(exe):
    qs = list(compact_queries())
    got = run(exe, text="".join("C %d %d %d %d %d %d %d %d 8 4 1\n" % q for q in qs)).splitlines()
    # 4 device sizes x 7 frame counts x 192 settings x the ROI sizes of each (cu, n): 45 + 5, less the sizes below 1 where
    # cap // n is 0 (n = cap + 1) and the coincidences among the rest
    assert len(got) == len(qs) == 192 * sum(len(roi_sizes(4 * cu, n)) for cu in CUS for n in (1, 2, 3, 4, 5, 16, 4 * cu + 1))
    assert len(qs) == 248_832
    seen, totals = set(), set()
    for q, line in zip(qs, got):
        cu, algo, force, rpxt, form, captured, n, roi_n = q
        want = rm.compact_plan(algo, roi_n, n, 8, rpxt, form, cu, bool(captured), force)
        split, a, pxt, f, grid, stagger, clean = (int(x) for x in line.split()[1:])
        if want.split:
            assert split == 1, (q, line)
            seen.add("split")
            continue
        assert (split, a, pxt, grid, stagger, clean) == (0, want.algo, want.pxt, want.grid, int(want.stagger), int(want.self_clean)), (q, line, want)
        assert a != 2 or f == want.form, (q, line, want)
        seen.add(a)
        if a == 3 and stagger:
            seen.add("ramp")
        if a == 1 and (force or algo) == 2:
            seen.add("more frames than blocks")
        if a != 3 and (force or algo) == 3:
            seen.add("resident asked for, not possible")
        if not (algo or force) and not captured:
            totals.add((n, rm.tiles_of(roi_n, 8) * n, a))
    assert {1, 2, 3, "split", "ramp", "more frames than blocks", "resident asked for, not possible"} <= seen, seen
    # the big-batch seam: 4 x 5,120 = 20,480 tiles go to the single pass, 4 x 5,119 do not, and 3 frames never do
    assert {(4, 20480, 2), (4, 20484, 2), (3, 20481, 1), (3, 20478, 1)} <= totals and not any(t == (4, 20476, 2) for t in totals), totals
    assert not any(n < 4 and a == 2 for n, _, a in totals)


def callback_queries():
    for cu, per_cu, form, tx, ty in itertools.product(CUS, (1, 2, 3), (1, 2), (1, 2, 5, 127, 128), (1, 3, 130)):
        nfc = max(cu * per_cu // (tx + 1), 1)
        for n in sorted({1, nfc - 1, nfc, nfc + 1, 2 * nfc - 1, 2 * nfc, 2 * nfc + 1} - {0, -1}):
            yield cu, per_cu, form, tx, ty, n


def test_callback_compact_plans_equal_the_model(exe):
    qs = list(callback_queries())
    got = run(exe, text="".join("B %d %d %d %d %d %d\n" % q for q in qs)).splitlines()
    assert len(got) == len(qs) and len(qs) == 2_124      # 360 settings x at most 7 frame counts, fewer where nfc is 1 or 2
    seen = set()
    for q, line in zip(qs, got):
        cu, per_cu, form, tx, ty, n = q
        want = rm.callback_plan(cu, per_cu, tx, ty, n, form)
        head, first, last = line[2:].split("|")
        assert tuple(map(int, head.split())) == (want.resident, want.nfc, len(want.subs)), (q, line, want)
        assert tuple(map(int, first.split())) == (want.subs[0].per_frame, want.subs[0].grid, int(want.subs[0].pipelined)), (q, line, want)
        assert tuple(map(int, last.split())) == (want.subs[-1].ns, want.subs[-1].per_frame, want.subs[-1].grid, int(want.subs[-1].pipelined)), (q, line, want)
        assert sum(s.ns for s in want.subs) == n
        seen |= {("pipelined", s.pipelined) for s in want.subs} | {("subs", len(want.subs))}
        if form == 2 and not want.subs[0].pipelined:
            seen.add("form 2 falls to one tile per block")
    assert {("pipelined", True), ("pipelined", False), ("subs", 1), ("subs", 2), ("subs", 3), "form 2 falls to one tile per block"} <= seen, seen


def test_the_route_of_the_gpu_cases_is_the_plan_s(exe):
    """callback_route -- what test_callback_compact_occupancy_gpu.py asserts per case -- is callback_plan's first
    sub-batch; `route` is compact_plan's launch."""
    for (roi_w, roi_h), per_cu, aim, cu in itertools.product(((1031, 250), (4097, 96), (256, 6400), (672, 400)), (1, 3), (0, 6, 32), CUS):
        if cu < aim:       # (no frame at all)
            continue
        r = rm.callback_route(roi_w, roi_h, per_cu, aim, cu)
        p = rm.callback_plan(cu, per_cu, r.tiles_x, r.tiles_y, r.n)
        assert (r.resident, r.nfc, r.sub_batches) == (p.resident, p.nfc, len(p.subs))
        assert r.pipelined == p.subs[0].pipelined and (not r.pipelined or r.per_frame == p.subs[0].per_frame)
    for algo, roi_n, n in itertools.product(range(5), (2047, 2048 * 1024, 2048 * 1025, 2048 * 5120), (1, 3, 4)):
        p = rm.compact_plan(algo, roi_n, n)
        assert not p.split and rm.route(algo, roi_n, n) == (p.algo, p.pxt, p.tiles)


def test_overlap_and_parity_seams_equal_the_model(exe):
    qs, want = [], []
    floor = 16 << 20
    for chunks, n, median, bridge16, captured in itertools.product((0, 1, 2, 4), (1, 2, 16), (0, 1), (0, 1), (0, 1)):
        c = max(min(chunks, n), 1)
        for px in (-(-floor * c // n) - 4096, -(-floor * c // n), -(-floor * c // n) + 4096):   # pixels per frame: width 4096
            h = -(-px // 4096)
            for fused, fused_compact, compact, bs, roi_w in itertools.product((0, 1), (0, 1, 2), (0, 1), (0, 1), (128 * 256, 128 * 256 + 1)):
                qs.append("O %d %d %d 4096 %d %d %d %d %d %d %d %d\n" % (chunks, fused, fused_compact, h, n, median, bridge16, captured, compact, bs, roi_w))
                overlap, chunk = rm.callback_overlap(chunks, 4096, h, n, median, bridge16, captured)
                want.append("O %d %d %d" % (overlap, chunk, rm.callback_one_kernel(overlap, median, fused, fused_compact, compact, bs, roi_w)))
    for forced, f32, n in itertools.product((0, 4), (0, 1), (11, 12, 13)):       # 12 x 4,000 x 2,000 = 96,000,000 pixels
        qs.append("P %d %d 40 4080 2080 %d\n" % (forced, f32, n))
        want.append("P %d" % (forced or (2 if f32 or n < 12 else 1)))
    got = run(exe, text="".join(qs)).splitlines()
    assert len(got) == len(qs) == 4 * 3 * 8 * 3 * 48 + 12
    assert got == want, [(q, g, w) for q, g, w in zip(qs, got, want) if g != w][:5]
    assert {w for w in want if w[0] == "O"} >= {"O 1 1 0", "O 1 8 0", "O 0 16 1", "O 0 16 0"}
