"""The terrain session of the obstacle sectors (d2pc_sectors_terrain_*) without a GPU: the header, the binding and the exports
agree on the new symbols; the struct sizes and defaults; the refusals of geometry, create and d2pc_sectors_terrain_desc_check
through the library and again through a stand-alone program under sanitizers; and tests/sectors_terrain_ref.py against a
brute-force dictionary of world cells over random scroll sequences.  tests/README_sectors_terrain.md has the map."""
import collections
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ground_ref as gref
import sectors_terrain_ref as tref
from disparity_to_point_cloud_amd import sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, NO_DEVICE = 1, 3, 5
F32 = np.float32
TERRAIN_SYMBOLS = ["d2pc_sectors_terrain_config_init", "d2pc_sectors_terrain_create", "d2pc_sectors_terrain_desc_check",
                   "d2pc_sectors_terrain_desc_init", "d2pc_sectors_terrain_destroy", "d2pc_sectors_terrain_geometry",
                   "d2pc_sectors_terrain_last_error", "d2pc_sectors_terrain_reset_device", "d2pc_sectors_terrain_state",
                   "d2pc_sectors_terrain_update_device"]


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_hold_the_terrain_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d2pc_sectors.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))
    assert sorted(n for n in declared if "_terrain_" in n) == TERRAIN_SYMBOLS
    assert sorted(n for n in sectors.SECTORS_SYMBOLS if "_terrain_" in n) == TERRAIN_SYMBOLS
    assert not [n for n in TERRAIN_SYMBOLS if "_ground_" in n or "_memory_" in n or "_steer_" in n or not n.startswith("d2pc_sectors_")]
    lib = d2pc.load_sectors_library()
    out = subprocess.run(["nm", "-D", "--defined-only", d2pc.sectors_library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    for name in TERRAIN_SYMBOLS:
        assert hasattr(lib, name) and name in exported, name
    assert d2pc.SectorsTerrain is sectors.SectorsTerrain
    for name in ("SectorsTerrainConfig", "SectorsTerrainDesc", "SectorsTerrainGeometry", "sectors_terrain_config_init",
                 "sectors_terrain_desc_init", "sectors_terrain_desc_check", "sectors_terrain_geometry"):
        assert getattr(d2pc, name) is getattr(sectors, name), name
    # the libraries stay apart: the product library holds nothing of the terrain
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(os.path.dirname(d2pc.sectors_library_path()), "libd2pc.so")],
                         capture_output=True, text=True, check=True).stdout
    assert "terrain" not in out


def test_struct_sizes_defaults_and_null_sessions(tmp_path):
    sizes = dict(d2pc_sectors_terrain_config=(d2pc.SectorsTerrainConfig, 32), d2pc_sectors_terrain_geometry_t=(d2pc.SectorsTerrainGeometry, 64),
                 d2pc_sectors_terrain_desc=(d2pc.SectorsTerrainDesc, 128))
    for name, (cls, size) in sizes.items():
        assert ctypes.sizeof(cls) == size, name
    src = tmp_path / "sizes.c"
    src.write_text('#include "d2pc_sectors.h"\n' + "".join(
        "typedef char size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (n, n, s) for n, (_, s) in sizes.items()) +
        "typedef char caps[D2PC_SECTORS_TERRAIN_MAX_DEPTH == 16 && D2PC_SECTORS_TERRAIN_HEADER_BYTES == 16 && "
        "D2PC_SECTORS_TERRAIN_MAX_CORNER == 536870912 ? 1 : -1];\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "sizes.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert (sectors.TERRAIN_MAX_DEPTH, sectors.TERRAIN_HEADER_BYTES, sectors.TERRAIN_MAX_CORNER) == (16, 16, 1 << 29)
    c = d2pc.sectors_terrain_config_init()
    assert (c.struct_size, c.depth, list(c.reserved)) == (32, 8, [0] * 6)
    d = d2pc.sectors_terrain_desc_init()
    assert (d.struct_size, d.n_candidates) == (128, 1) and all(getattr(d, k) is None for k, _ in d._fields_[2:])
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_terrain_config_init(None)   # tolerated
    lib.d2pc_sectors_terrain_desc_init(None)
    assert lib.d2pc_sectors_terrain_last_error(None) == b"null session"
    p, n = ctypes.c_void_p(0x55), ctypes.c_size_t(7)
    assert lib.d2pc_sectors_terrain_state(None, ctypes.byref(p), ctypes.byref(n)) == INVALID_ARG and (p.value, n.value) == (0x55, 7)
    assert lib.d2pc_sectors_terrain_destroy(None) == INVALID_ARG and lib.d2pc_sectors_terrain_reset_device(None, None) == INVALID_ARG
    assert lib.d2pc_sectors_terrain_update_device(None, ctypes.byref(d), None) == INVALID_ARG


# ------------------------------------------------------------------------------------------------------ refusals
def test_geometry_and_create_refusals_and_no_device():
    lib = d2pc.load_sectors_library()
    h, g = ctypes.c_void_p(), d2pc.SectorsTerrainGeometry()
    no_gpu = d2pc.device_count() == 0
    ok = NO_DEVICE if no_gpu else 0

    def status(ground=None, struct_size=32, reserved=None, **kw):
        gc = d2pc.sectors_ground_config_init(**(ground or {}))
        c = d2pc.sectors_terrain_config_init(**kw)
        c.struct_size = struct_size
        if reserved is not None:
            c.reserved[reserved] = 1
        st = lib.d2pc_sectors_terrain_create(ctypes.byref(gc), ctypes.byref(c), ctypes.byref(h))
        if h:
            lib.d2pc_sectors_terrain_destroy(h)
        ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
        refused = lib.d2pc_sectors_terrain_geometry(ctypes.byref(gc), ctypes.byref(c), ctypes.byref(g))
        assert (st in (0, NO_DEVICE)) == (refused == 0) and (refused == 0 or st == refused), "create refuses what geometry refuses"
        if refused:
            assert bytes(g) == b"\xa5" * ctypes.sizeof(g) and not h, "a refused call wrote"
            desc = d2pc.sectors_terrain_desc_init(step=0x1000, frame_count=0x2000, frame_sum=0x3000, frame_sum2=0x4000, status=0x5000)
            assert d2pc.sectors_terrain_desc_check(gc, c, desc) == refused, "desc_check refuses a configuration as create does"
            gg = d2pc.SectorsGroundGeometry()
            ground_refused = lib.d2pc_sectors_ground_geometry(ctypes.byref(gc), ctypes.byref(gg))
            assert ground_refused in (0, refused), "the ground configuration's refusals come first, unchanged"
        return st

    gc, tc = d2pc.sectors_ground_config_init(), d2pc.sectors_terrain_config_init()
    assert lib.d2pc_sectors_terrain_create(ctypes.byref(gc), ctypes.byref(tc), None) == INVALID_ARG
    assert lib.d2pc_sectors_terrain_create(None, ctypes.byref(tc), ctypes.byref(h)) == INVALID_ARG and not h
    assert lib.d2pc_sectors_terrain_create(ctypes.byref(gc), None, ctypes.byref(h)) == INVALID_ARG and not h
    assert lib.d2pc_sectors_terrain_geometry(ctypes.byref(gc), ctypes.byref(tc), None) == INVALID_ARG
    assert lib.d2pc_sectors_terrain_geometry(ctypes.byref(gc), None, ctypes.byref(g)) == INVALID_ARG
    assert lib.d2pc_sectors_terrain_geometry(None, ctypes.byref(tc), ctypes.byref(g)) == INVALID_ARG
    assert status() == ok and status(depth=1) == ok and status(depth=16, ground=dict(n_a=64, n_b=64)) == ok
    assert status(struct_size=28) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for depth in (0, -1, 17, 1 << 20):
        assert status(depth=depth) == BAD_SIZE, depth
    for r in range(6):
        assert status(reserved=r) == INVALID_ARG, r
    assert status(depth=17, reserved=2) == BAD_SIZE and status(depth=17, struct_size=0) == INVALID_ARG, "in the order the header lists them"
    # the ground configuration's refusals, first
    assert status(ground=dict(quantum=0.0), depth=17) == INVALID_ARG and status(ground=dict(n_a=65), struct_size=0) == BAD_SIZE
    assert status(ground=dict(window=9), reserved=0) == BAD_SIZE and status(ground=dict(min_count=0)) == INVALID_ARG
    if no_gpu:
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.SectorsTerrain(d2pc.sectors_ground_config_init())
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_ground_config_init(device_id=1 << 20)
    assert lib.d2pc_sectors_terrain_create(ctypes.byref(bad), ctypes.byref(tc), ctypes.byref(h)) == NO_DEVICE and not h


def test_geometry_sizes():
    for n_a, n_b, depth in ((2, 2, 1), (5, 3, 3), (16, 16, 8), (33, 31, 2), (32, 32, 16), (33, 32, 4), (64, 64, 16)):
        gc = d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b, cell_size=0.25)
        g = d2pc.sectors_terrain_geometry(gc, d2pc.sectors_terrain_config_init(depth=depth))
        n = n_a * n_b
        assert (g.n_cells, g.inv_c, g.headers_offset, g.tables_offset, list(g.reserved)) == (n, 4.0, 0, 256, [0] * 6)
        assert g.slot_bytes == tref.slot_bytes(n) == (20 * n + 15) // 16 * 16 and g.state_bytes == 256 + depth * g.slot_bytes
    assert tref.slot_bytes(15) == 304 and tref.slot_bytes(1023) == 20464 and tref.slot_bytes(4096) == 81920
    assert d2pc.sectors_terrain_geometry(d2pc.sectors_ground_config_init(cell_size=0.3), d2pc.sectors_terrain_config_init()).inv_c == \
        d2pc.sectors_ground_geometry(d2pc.sectors_ground_config_init(cell_size=0.3)).inv_c


# name -> (base address, bytes per cell, fixed bytes, alignment)
BUFFERS = dict(step=(0x40000000, 0, 80, 4), frame_count=(0x40100000, 4, 0, 4), frame_sum=(0x40200000, 8, 0, 8), frame_sum2=(0x40300000, 8, 0, 8),
               allowed=(0x40400000, 1, 0, 1),
               count=(0x50000000, 4, 0, 4), sum=(0x50100000, 8, 0, 8), sum2=(0x50200000, 8, 0, 8), mean_q=(0x50300000, 4, 0, 4),
               spread_q2=(0x50400000, 4, 0, 4), flat=(0x50500000, 1, 0, 1), site=(0x50600000, 1, 0, 1), candidates=(0x50700000, 0, 40, 8),
               summary=(0x50800000, 0, 16, 4), status=(0x50900000, 0, 16, 4))
OUTPUTS = ("count", "sum", "sum2", "mean_q", "spread_q2", "flat", "site", "candidates", "summary", "status")


@pytest.mark.parametrize("grid", [dict(), dict(n_a=64, n_b=64), dict(n_a=5, n_b=3)], ids=["256", "4096", "15"])
def test_desc_refusals_without_a_device(grid):
    """d2pc_sectors_terrain_desc_check is d2pc_sectors_terrain_update_device's own check (csrc/d2pc_sectors_terrain_plan.hpp);
    the pointers are numbers here, nothing is dereferenced."""
    cfg, tcfg = d2pc.sectors_ground_config_init(**grid), d2pc.sectors_terrain_config_init(depth=3)
    n = cfg.n_a * cfg.n_b
    good = dict({k: v[0] for k, v in BUFFERS.items()}, n_candidates=5)
    size = {k: per * n + fixed for k, (_, per, fixed, _) in BUFFERS.items()}

    def status(cfg=cfg, tcfg=tcfg, **kw):
        return d2pc.sectors_terrain_desc_check(cfg, tcfg, d2pc.sectors_terrain_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    desc = d2pc.sectors_terrain_desc_init(**good)
    assert status() == 0 and status(allowed=None) == 0
    assert lib.d2pc_sectors_terrain_desc_check(ctypes.byref(cfg), ctypes.byref(tcfg), None) == INVALID_ARG
    assert lib.d2pc_sectors_terrain_desc_check(None, ctypes.byref(tcfg), ctypes.byref(desc)) == INVALID_ARG
    assert lib.d2pc_sectors_terrain_desc_check(ctypes.byref(cfg), None, ctypes.byref(desc)) == INVALID_ARG
    assert status(cfg=d2pc.sectors_ground_config_init(n_a=65), step=None) == BAD_SIZE, "the configurations' refusals come first"
    assert status(tcfg=d2pc.sectors_terrain_config_init(depth=0), step=None) == BAD_SIZE
    # each alone
    assert status(struct_size=120) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for k in ("step", "frame_count", "frame_sum", "frame_sum2"):
        assert status(**{k: None}) == INVALID_ARG, k
    assert status(**{k: None for k in OUTPUTS}) == INVALID_ARG
    for only in OUTPUTS:
        assert status(**{k: (good[k] if k == only else None) for k in OUTPUTS}) == 0, only
    for k in (0, -1, 33, 1 << 20):
        assert status(n_candidates=k) == INVALID_ARG, k
        assert status(n_candidates=k, candidates=None) == 0, "n_candidates is not looked at without candidates"
    assert status(n_candidates=1) == 0 and status(n_candidates=32) == 0
    # alignment to the type; the 64-bit tables and candidates to 8 bytes
    for k, (base, _, _, align) in BUFFERS.items():
        for off in range(1, align):
            assert status(**{k: base + off}) == INVALID_ARG, (k, off)
        assert status(**{k: base + align}) == 0, k
    # overlap: every output over the first and over the last byte of every other buffer
    for o in OUTPUTS:
        align = BUFFERS[o][3]
        for b, (base, _, _, _) in BUFFERS.items():
            if b == o:
                continue
            end = base + size[b]
            lo, last, hi = base - size[o], (end - 1) // align * align, (end + align - 1) // align * align
            if lo % align:                       # (an odd number of cells: keep the pointer aligned)
                lo -= lo % align
            assert status(**{o: lo + align}) == INVALID_ARG, (o, "over the first byte of", b)
            assert status(**{o: lo}) == 0, (o, "ends before", b, "begins")
            assert status(**{o: last}) == INVALID_ARG, (o, "over the last byte of", b)
            assert status(**{o: hi}) == 0, (o, "begins where", b, "ends")
    assert status(allowed=None, summary=BUFFERS["allowed"][0]) == 0, "a buffer that is not given overlaps nothing"
    assert status(count=BUFFERS["frame_count"][0]) == INVALID_ARG, "in place is refused"
    ca = BUFFERS["candidates"][0]
    assert status(n_candidates=1, summary=ca + 8) == 0 and status(n_candidates=2, summary=ca + 8) == INVALID_ARG
    assert status(n_candidates=32, summary=ca + 248) == INVALID_ARG and status(n_candidates=32, summary=ca + 256) == 0


def test_terrain_plan_header_compiles_with_plain_gxx_and_runs_under_sanitizers(tmp_path):
    """csrc/d2pc_sectors_terrain_plan.hpp holds no HIP; tests/cpp/sectors_terrain_plan_main.cpp, a stand-alone program over it
    (host code, nothing loaded into Python), runs the refusal matrices, the sizes and the state overlap with
    -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc")
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(csrc, "d2pc_sectors_terrain_plan.hpp")).read()).lower()
    one = tmp_path / "one.cpp"
    one.write_text('#include "d2pc_sectors_terrain_plan.hpp"\nint main() { d2pc::sectors::TerrainPlan p; '
                   'return d2pc::sectors::make_terrain_plan(nullptr, nullptr, &p) == 1 ? 0 : 1; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", csrc, str(one), "-o", str(tmp_path / "one")],
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    assert subprocess.run([str(tmp_path / "one")], timeout=60).returncode == 0
    exe = tmp_path / "sectors_terrain_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "sectors_terrain_plan_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------------------------- the reference itself
def random_tables(rng, n, fill=0.7, k_range=200):
    """Tables a ground call could have written: a few heights per cell."""
    count, total, total2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.uint64)
    for c in np.flatnonzero(rng.random(n) < fill):
        ks = rng.integers(-k_range, k_range + 1, int(rng.integers(1, 6)))
        count[c], total[c], total2[c] = len(ks), int(ks.sum()), int((ks * ks).sum())
    return count, total, total2


def test_anchor_rounds_half_to_even_and_gates_in_float():
    def anc(a0, b0=0.0, inv_c=1.0):
        return tref.anchor(gref.step_words(np.eye(3), np.zeros(3), [a0, b0, 0.0]), inv_c)

    assert anc(2.5) == (True, 2, 0) and anc(3.5) == (True, 4, 0) and anc(-0.5) == (True, 0, 0) and anc(-1.5) == (True, -2, 0)
    assert anc(1.25, -1.75, 2.0) == (True, 2, -4), "2.5 -> 2 and -3.5 -> -4"
    assert anc(536870912.0) == (True, 1 << 29, 0) and anc(-536870912.0, 536870912.0) == (True, -(1 << 29), 1 << 29)
    beyond = float(np.nextafter(F32(536870912.0), F32(np.inf)))
    assert anc(beyond) == (False, 0, 0) and anc(0.0, -beyond) == (False, 0, 0)
    for bad in (np.nan, np.inf, -np.inf):
        assert anc(bad) == (False, 0, 0) and anc(0.0, bad) == (False, 0, 0)
    assert anc(3e38, 0.0, 2.0) == (False, 0, 0), "the product overflows to inf"


def test_cell_outputs_equal_the_ground_references_from_points():
    rng = np.random.default_rng(3)
    cfg = d2pc.sectors_ground_config_init(n_a=20, n_b=10, min_count=2, max_spread_q2=5000)
    ref = gref.SectorsGroundRef(cfg, d2pc.sectors_ground_geometry(cfg))
    cell = rng.integers(0, 180, 3000)
    k = np.where(rng.random(3000) < 0.2, rng.integers(-32767, 32768, 3000), rng.integers(-60, 60, 3000))
    want = ref.cells(cell, k)
    mean, spread, flat = tref.cell_outputs(want["count"], want["sum"].view(np.uint64), want["sum2"], 2, 5000)
    assert np.array_equal(mean, want["mean_q"]) and np.array_equal(spread, want["spread_q2"]) and np.array_equal(flat, want["flat"])
    assert (want["count"] == 0).any() and flat.any() and (mean < 0).any()


@pytest.mark.parametrize("n_a,n_b,depth", [(5, 3, 3), (8, 6, 1), (7, 9, 4), (4, 4, 16)])
def test_reference_against_a_dictionary_of_world_cells(n_a, n_b, depth):
    """Random scroll sequences: the window of the reference equals sums over a dictionary keyed by WORLD cell, kept per frame
    for the last `depth` anchored frames -- no ring, no slot, no shifted index.  Frames that are not anchored, changes of h0
    and jumps that leave no overlap are among the steps."""
    rng = np.random.default_rng(1000 * n_a + 10 * n_b + depth)
    cfg = d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b, cell_size=0.5, min_count=2, max_spread_q2=20000, window=1, max_step_q=150)
    ref = tref.SectorsTerrainRef(cfg, d2pc.sectors_ground_geometry(cfg), depth)
    n = n_a * n_b
    frames = collections.deque(maxlen=depth)             # (h0 bits as float, {world cell: (count, sum, sum2)})
    ia, jb, h0, seq = 0, 0, 1.0, 0
    dropped = shifted = unanchored = 0
    for it in range(60):
        r = rng.random()
        if r < 0.5:
            ia, jb = ia + int(rng.integers(-2, 3)), jb + int(rng.integers(-2, 3))
        elif r < 0.6:
            ia, jb = ia + int(rng.integers(-n_a - 1, n_a + 2)), jb + int(rng.integers(-n_b - 1, n_b + 2))
        elif r < 0.7:
            h0 = float(rng.choice([1.0, 2.0]))
        corner = [0.5 * ia, 0.5 * jb, h0]
        if r > 0.93:
            corner[int(rng.integers(0, 2))] = float(rng.choice([np.nan, np.inf, 4e8]))      # 4e8 x 2 > 2^29
        step = gref.step_words(np.eye(3), np.zeros(3), corner, int(rng.integers(0, n_a)), int(rng.integers(0, n_b)))
        count, total, total2 = random_tables(rng, n)
        before = ref.state.copy()
        got = ref.update(step, count, total, total2, n_candidates=4)
        if r > 0.93:
            unanchored += 1
            assert np.array_equal(ref.state, before) and got["status"].tolist() == [seq, 0, 0, 0]
            assert not got["count"].any() and np.all(got["mean_q"] == -(1 << 31)) and np.all(got["candidates"] == gref.NO_CANDIDATE)
            continue
        seq += 1
        world = {}
        for c in np.flatnonzero(count):
            world[(ia + c % n_a, jb + c // n_a)] = (int(count[c]), int(total[c]), int(total2[c]))
        frames.append((h0, ia, jb, world))
        w_count, w_sum, w_sum2 = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
        took = 0
        for fh0, fia, fjb, fworld in frames:
            if fh0 != h0:
                dropped += 1
                continue
            if abs(fia - ia) >= n_a or abs(fjb - jb) >= n_b:
                continue                                  # no cell of the frame's grid is in sight
            took += 1
            shifted += (fia, fjb) != (ia, jb)
            for c in range(n):
                e = fworld.get((ia + c % n_a, jb + c // n_a))
                if e:
                    w_count[c] += e[0]
                    w_sum[c] += e[1]
                    w_sum2[c] += e[2]
        assert got["status"].tolist() == [seq, took, ia & 0xFFFFFFFF, jb & 0xFFFFFFFF], it
        assert np.array_equal(got["count"], w_count) and np.array_equal(got["sum"], w_sum) and np.array_equal(got["sum2"].astype(np.int64), w_sum2), it
        mean, spread, flat = tref.cell_outputs(w_count.astype(np.uint32), w_sum.view(np.uint64), w_sum2.astype(np.uint64), 2, 20000)
        assert np.array_equal(got["mean_q"], mean) and np.array_equal(got["spread_q2"], spread) and np.array_equal(got["flat"], flat)
        assert np.array_equal(got["site"], gref.brute_sites(n_a, n_b, 1, 150, mean, flat))
        assert got["summary"].tolist() == [int(w_count.sum()), int(flat.sum()), int(got["site"].sum()), 0]
    assert unanchored >= 1 and (depth == 1 or (shifted > 10 and dropped >= 1)), "depth 1 is the frame alone"


def test_reference_ring_wrap_and_restart():
    cfg = d2pc.sectors_ground_config_init(n_a=2, n_b=2, min_count=1)
    ref = tref.SectorsTerrainRef(cfg, d2pc.sectors_ground_geometry(cfg), 3)
    step = gref.step_words(np.eye(3), np.zeros(3), np.zeros(3))
    one = (np.array([1, 0, 0, 0], dtype=np.uint32), np.array([7, 0, 0, 0], dtype=np.int64), np.array([49, 0, 0, 0], dtype=np.uint64))
    slots = []
    for it in range(7):
        got = ref.update(step, *one)
        slots.append(int(np.argmax(ref.headers()[:3, 3])))
        assert got["status"].tolist() == [it + 1, min(it + 1, 3), 0, 0] and got["count"][0] == min(it + 1, 3)
    assert slots == [0, 1, 2, 0, 1, 2, 0], "the smallest seq is replaced, the lowest index on a tie"
    assert ref.headers()[3:].sum() == 0, "headers at and beyond depth stay zero"
    # two counts of 2^31 wrap to an empty cell
    big = (np.array([0x80000000, 1, 0, 0], dtype=np.uint32), np.zeros(4, dtype=np.int64), np.zeros(4, dtype=np.uint64))
    ref.reset()
    ref.update(step, *big)
    got = ref.update(step, *big)
    assert got["count"].tolist() == [0, 2, 0, 0] and got["mean_q"][0] == -(1 << 31) and got["spread_q2"][0] == 0xFFFFFFFF and got["flat"].tolist() == [0, 1, 0, 0]
    # seq 0xFFFFFFFF restarts: the other headers are stored as zeros
    ref.headers()[1, 3] = 0xFFFFFFFF
    got = ref.update(step, *one)
    assert got["status"].tolist() == [1, 1, 0, 0] and got["count"].tolist() == [1, 0, 0, 0]
    assert ref.headers()[:3, 3].tolist() == [1, 0, 0] and not ref.headers()[1:].any()
    got = ref.update(step, *one)
    assert got["status"].tolist() == [2, 2, 0, 0] and ref.headers()[:3, 3].tolist() == [1, 2, 0]
