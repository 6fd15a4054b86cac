"""The landing grid of the obstacle sectors (d2pc_sectors_ground_*) without a GPU: the header, the binding and the exports
agree on the new symbols; the struct sizes and defaults; the refusals of create and of d2pc_sectors_ground_desc_check through
the library and again through a stand-alone program under sanitizers; geometry and the block count; spread_of_std; and
tests/sectors_ground_ref.py against float64 binning, against the wrapped formula for S, against a brute-force window and on
the candidates' order.  tests/README_sectors_ground.md has the map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ground_ref as gref
from disparity_to_point_cloud_amd import sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, NO_DEVICE = 1, 3, 5
F32 = np.float32
GROUND_SYMBOLS = ["d2pc_sectors_ground_blocks", "d2pc_sectors_ground_config_init", "d2pc_sectors_ground_create",
                  "d2pc_sectors_ground_desc_check", "d2pc_sectors_ground_desc_init", "d2pc_sectors_ground_destroy",
                  "d2pc_sectors_ground_geometry", "d2pc_sectors_ground_last_error", "d2pc_sectors_ground_process_device",
                  "d2pc_sectors_ground_spread_of_std"]


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_hold_the_ground_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d2pc_sectors.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))
    assert sorted(n for n in declared if "_ground_" in n) == GROUND_SYMBOLS
    assert sorted(n for n in sectors.SECTORS_SYMBOLS if "_ground_" in n) == GROUND_SYMBOLS
    assert not [n for n in GROUND_SYMBOLS if "_memory_" in n or "_steer_" in n or not n.startswith("d2pc_sectors_")]
    lib = d2pc.load_sectors_library()
    out = subprocess.run(["nm", "-D", "--defined-only", d2pc.sectors_library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    for name in GROUND_SYMBOLS:
        assert hasattr(lib, name) and name in exported, name
    assert d2pc.SectorsGround is sectors.SectorsGround
    for name in ("SectorsGroundConfig", "SectorsGroundDesc", "SectorsGroundGeometry", "SectorsGroundStep", "sectors_ground_config_init",
                 "sectors_ground_desc_init", "sectors_ground_desc_check", "sectors_ground_geometry", "sectors_ground_spread_of_std",
                 "sectors_ground_step"):
        assert getattr(d2pc, name) is getattr(sectors, name), name


def test_struct_sizes_defaults_and_null_sessions(tmp_path):
    sizes = dict(d2pc_sectors_ground_config=(d2pc.SectorsGroundConfig, 80), d2pc_sectors_ground_geometry_t=(d2pc.SectorsGroundGeometry, 64),
                 d2pc_sectors_ground_step=(d2pc.SectorsGroundStep, 80), d2pc_sectors_ground_desc=(d2pc.SectorsGroundDesc, 136),
                 d2pc_sectors_ground_candidate=(d2pc.SectorsSteerCandidate, 8))
    for name, (cls, size) in sizes.items():
        assert ctypes.sizeof(cls) == size, name
    src = tmp_path / "sizes.c"
    src.write_text('#include "d2pc_sectors.h"\n' + "".join(
        "typedef char size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (n, n, s) for n, (_, s) in sizes.items()) +
        "typedef char caps[D2PC_SECTORS_GROUND_MAX_CELLS_PER_AXIS == 64 && D2PC_SECTORS_GROUND_MAX_WINDOW == 8 && "
        "D2PC_SECTORS_GROUND_MAX_CANDIDATES == 32 && D2PC_SECTORS_GROUND_MAX_WEIGHT == 4095 && D2PC_SECTORS_GROUND_MAX_K == 32767 && "
        "D2PC_SECTORS_GROUND_EMPTY_MEAN == 0x80000000u && D2PC_SECTORS_GROUND_EMPTY_SPREAD == 0xFFFFFFFFu && "
        "D2PC_SECTORS_GROUND_OFF == 0xFFFFFFFFu ? 1 : -1];\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "sizes.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert (sectors.GROUND_MAX_CELLS_PER_AXIS, sectors.GROUND_MAX_WINDOW, sectors.GROUND_MAX_CANDIDATES, sectors.GROUND_MAX_WEIGHT,
            sectors.GROUND_MAX_K, sectors.GROUND_EMPTY_MEAN, sectors.GROUND_EMPTY_SPREAD, sectors.GROUND_OFF) == (
                64, 8, 32, 4095, 32767, 0x80000000, 0xFFFFFFFF, 0xFFFFFFFF)
    c = d2pc.sectors_ground_config_init()
    assert (c.struct_size, c.device_id, c.n_a, c.n_b, c.cell_size, F32(c.quantum), list(c.axes), c.min_count, c.max_spread_q2, c.max_step_q,
            c.window, c.w_dist, c.w_rough, c.rough_cap, c.max_points, list(c.reserved)) == (
                80, 0, 16, 16, 0.5, F32(0.002), [1, 2, 3], 4, 625, 50, 1, 1, 1, 65535, 0, [0, 0, 0])
    d = d2pc.sectors_ground_desc_init()
    assert (d.struct_size, d.point_step, d.n_clouds, d.n_candidates, d.cloud_points, d.points_frame_stride_points) == (136, 16, 1, 1, 0, 0)
    assert all(getattr(d, k) is None for k, _ in d._fields_[4:] if k not in ("cloud_points", "points_frame_stride_points"))
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_ground_config_init(None)   # tolerated
    lib.d2pc_sectors_ground_desc_init(None)
    assert lib.d2pc_sectors_ground_last_error(None) == b"null session" and lib.d2pc_sectors_ground_blocks(None) == 0
    assert lib.d2pc_sectors_ground_destroy(None) == INVALID_ARG and lib.d2pc_sectors_ground_process_device(None, ctypes.byref(d), None) == INVALID_ARG
    R = np.arange(9, dtype=F32)
    w = d2pc.sectors_ground_step(R, [10, 11, 12], [0.5, -0.5, 100.0], 3, 0xFFFFFFFF)
    assert w.dtype == np.uint32 and len(w) == 20 and np.array_equal(w, gref.step_words(R, [10, 11, 12], [0.5, -0.5, 100.0], 3, 0xFFFFFFFF))
    assert w[:15].view(F32).tolist() == list(range(9)) + [10, 11, 12, 0.5, -0.5, 100.0] and w[15:].tolist() == [3, 0xFFFFFFFF, 0, 0, 0]
    assert d2pc.sectors_ground_step(np.eye(3), [0, 0, 0], [0, 0, 0])[15:17].tolist() == [0xFFFFFFFF, 0xFFFFFFFF]


# ------------------------------------------------------------------------------------------------------ refusals
def test_create_refusals_and_no_device():
    lib = d2pc.load_sectors_library()
    h, g = ctypes.c_void_p(), d2pc.SectorsGroundGeometry()
    no_gpu = d2pc.device_count() == 0
    ok = NO_DEVICE if no_gpu else 0

    def status(struct_size=80, reserved=None, **kw):
        c = d2pc.sectors_ground_config_init(**kw)
        c.struct_size = struct_size
        if reserved is not None:
            c.reserved[reserved] = 1
        st = lib.d2pc_sectors_ground_create(ctypes.byref(c), ctypes.byref(h))
        if h:
            lib.d2pc_sectors_ground_destroy(h)
        ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
        refused = lib.d2pc_sectors_ground_geometry(ctypes.byref(c), ctypes.byref(g))
        assert (st in (0, NO_DEVICE)) == (refused == 0) and (refused == 0 or st == refused), "create refuses what geometry refuses"
        if refused:
            assert bytes(g) == b"\xa5" * ctypes.sizeof(g) and not h, "a refused call wrote"
            desc = d2pc.sectors_ground_desc_init(points=0x1000, cloud_points=4, step=0x2000, summary=0x3000)
            assert d2pc.sectors_ground_desc_check(c, desc) == refused, "desc_check refuses a configuration as create does"
        return st

    good = d2pc.sectors_ground_config_init()
    assert lib.d2pc_sectors_ground_create(ctypes.byref(good), None) == INVALID_ARG
    assert lib.d2pc_sectors_ground_create(None, ctypes.byref(h)) == INVALID_ARG and not h
    assert lib.d2pc_sectors_ground_geometry(ctypes.byref(good), None) == INVALID_ARG
    assert status() == ok and status(n_a=2, n_b=64, window=8) == ok and status(n_a=64, n_b=64, window=0, max_points=360960) == ok
    assert status(w_dist=4095, w_rough=4095, rough_cap=65535, max_step_q=65535, max_spread_q2=0xFFFFFFFF, min_count=0xFFFFFFFF) == ok
    assert status(w_dist=0, w_rough=0, rough_cap=0, max_step_q=0, max_spread_q2=0, axes=(2, -1, -3)) == ok
    assert status(struct_size=76) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for kw in (dict(axes=(1, 1, 3)), dict(axes=(1, 2, 4)), dict(axes=(0, 2, 3)), dict(axes=(-(1 << 31), 2, 3)), dict(cell_size=0.0),
               dict(cell_size=-0.5), dict(cell_size=np.nan), dict(cell_size=np.inf), dict(quantum=0.0), dict(quantum=-0.002),
               dict(quantum=np.nan), dict(quantum=np.inf), dict(min_count=0), dict(max_step_q=65536), dict(w_dist=4096), dict(w_rough=4096),
               dict(rough_cap=65536), dict(reserved=0), dict(reserved=1), dict(reserved=2),
               dict(quantum=0.0, n_a=99), dict(w_dist=4096, window=9)):                  # INVALID_ARG comes before BAD_SIZE
        assert status(**kw) == INVALID_ARG, kw
    for kw in (dict(n_a=1), dict(n_a=65), dict(n_b=1), dict(n_b=65), dict(n_a=-16), dict(window=-1), dict(window=9),
               dict(cell_size=1e-45), dict(quantum=2e-39)):
        assert status(**kw) == BAD_SIZE, kw
    if no_gpu:
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.SectorsGround()
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_ground_config_init(device_id=1 << 20)
    assert lib.d2pc_sectors_ground_create(ctypes.byref(bad), ctypes.byref(h)) == NO_DEVICE and not h


# name -> (base address, bytes per cell, fixed bytes, alignment); points: 1,000 records
BUFFERS = dict(points=(0x40000000, 0, 16000, 16), counts=(0x40100000, 0, 4, 4), step=(0x40200000, 0, 80, 4), allowed=(0x40300000, 1, 0, 1),
               count=(0x50000000, 4, 0, 4), sum=(0x50100000, 8, 0, 8), sum2=(0x50200000, 8, 0, 8), mean_q=(0x50300000, 4, 0, 4),
               spread_q2=(0x50400000, 4, 0, 4), flat=(0x50500000, 1, 0, 1), site=(0x50600000, 1, 0, 1), candidates=(0x50700000, 0, 40, 8),
               summary=(0x50800000, 0, 16, 4))
OUTPUTS = ("count", "sum", "sum2", "mean_q", "spread_q2", "flat", "site", "candidates", "summary")


@pytest.mark.parametrize("grid", [dict(), dict(n_a=64, n_b=64), dict(n_a=5, n_b=3)], ids=["256", "4096", "15"])
def test_desc_refusals_without_a_device(grid):
    """d2pc_sectors_ground_desc_check is d2pc_sectors_ground_process_device's own check (csrc/d2pc_sectors_ground_plan.hpp);
    the pointers are numbers here, nothing is dereferenced."""
    cfg = d2pc.sectors_ground_config_init(**grid)
    n = cfg.n_a * cfg.n_b
    good = dict({k: v[0] for k, v in BUFFERS.items()}, n_candidates=5, cloud_points=1000)
    size = {k: per * n + fixed for k, (_, per, fixed, _) in BUFFERS.items()}

    def status(cfg=cfg, **kw):
        return d2pc.sectors_ground_desc_check(cfg, d2pc.sectors_ground_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    desc = d2pc.sectors_ground_desc_init(**good)
    assert status() == 0 and status(allowed=None, counts=None) == 0 and status(point_step=32) == 0
    assert lib.d2pc_sectors_ground_desc_check(ctypes.byref(cfg), None) == INVALID_ARG
    assert lib.d2pc_sectors_ground_desc_check(None, ctypes.byref(desc)) == INVALID_ARG
    assert status(cfg=d2pc.sectors_ground_config_init(n_a=65), points=None) == BAD_SIZE, "the configuration's refusals come first"
    assert status(cfg=d2pc.sectors_ground_config_init(quantum=0.0), cloud_points=0) == INVALID_ARG
    # each alone
    assert status(struct_size=128) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for kw in (dict(point_step=12), dict(point_step=0), dict(n_clouds=0), dict(n_clouds=65536), dict(points=None), dict(step=None)):
        assert status(**kw) == INVALID_ARG, kw
    assert status(**{k: None for k in OUTPUTS}) == INVALID_ARG
    for only in OUTPUTS:
        assert status(**{k: (good[k] if k == only else None) for k in OUTPUTS}) == 0, only
    for k in (0, -1, 33, 1 << 20):
        assert status(n_candidates=k) == INVALID_ARG, k
        assert status(n_candidates=k, candidates=None) == 0, "n_candidates is not looked at without candidates"
    assert status(n_candidates=1) == 0 and status(n_candidates=32) == 0
    # alignment to the type; sum, sum2 and candidates to 8 bytes, points to 16
    for k, (base, _, _, align) in BUFFERS.items():
        for off in range(1, align):
            assert status(**{k: base + off}) == INVALID_ARG, (k, off)
        assert status(**{k: base + align}) == 0, k
    # the cloud sizes
    assert status(cloud_points=0) == BAD_SIZE and status(cloud_points=1 << 32) == BAD_SIZE
    assert status(cloud_points=(1 << 32) - 1, points=0x7000_0000_0000) == 0, "2^32 - 1 records, placed beyond every other buffer"
    assert status(n_clouds=2, points_frame_stride_points=999) == BAD_SIZE and status(n_clouds=2, points_frame_stride_points=1000) == 0
    assert status(n_clouds=3, points_frame_stride_points=1 << 31) == BAD_SIZE
    assert status(cloud_points=0, step=None) == INVALID_ARG and status(cloud_points=0, sum=BUFFERS["sum"][0] + 4) == INVALID_ARG
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
    assert status(allowed=None, summary=BUFFERS["allowed"][0] + 4) == 0, "a buffer that is not given overlaps nothing"
    ca = BUFFERS["candidates"][0]
    assert status(n_candidates=1, summary=ca + 8) == 0 and status(n_candidates=2, summary=ca + 8) == INVALID_ARG
    assert status(n_candidates=32, summary=ca + 248) == INVALID_ARG and status(n_candidates=32, summary=ca + 256) == 0
    # the extent of points follows the clouds
    pt = BUFFERS["points"][0]
    assert status(n_clouds=3, points_frame_stride_points=5000, summary=pt + 16 * 10999) == INVALID_ARG
    assert status(n_clouds=3, points_frame_stride_points=5000, summary=pt + 16 * 11000) == 0
    assert status(point_step=32, summary=pt + 32 * 999) == INVALID_ARG and status(point_step=32, summary=pt + 32 * 1000) == 0


def test_ground_plan_header_compiles_with_plain_gxx_and_runs_under_sanitizers(tmp_path):
    """csrc/d2pc_sectors_ground_plan.hpp holds no HIP; tests/cpp/sectors_ground_plan_main.cpp, a stand-alone program over it
    (host code, nothing loaded into Python), runs both refusal matrices, the block counts and spread_of_std with
    -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc")
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(csrc, "d2pc_sectors_ground_plan.hpp")).read()).lower()
    one = tmp_path / "one.cpp"
    one.write_text('#include "d2pc_sectors_ground_plan.hpp"\nint main() { d2pc::sectors::GroundPlan p; return d2pc::sectors::make_ground_plan(nullptr, &p) == 1 ? 0 : 1; }\n')
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", csrc, str(one), "-o", str(tmp_path / "one")],
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    assert subprocess.run([str(tmp_path / "one")], timeout=60).returncode == 0
    exe = tmp_path / "sectors_ground_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "sectors_ground_plan_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------ geometry
def test_defaults_geometry_and_the_block_count():
    g = d2pc.sectors_ground_geometry(d2pc.sectors_ground_config_init())
    assert (g.n_cells, g.inv_c, g.share_points, g.blocks_per_cu, g.blocks, g.lds_bytes, g.block_bytes) == (256, 2.0, 1024, 4, 1024, 5120, 5120)
    assert F32(g.inv_q) == F32(1.0 / float(F32(0.002))) and g.device_bytes == 1024 * 5120 + 13 * 256 and list(g.reserved) == [0] * 4
    for n_a, n_b, per_cu in ((2, 2, 4), (5, 3, 4), (16, 16, 4), (32, 64, 4), (45, 45, 4), (46, 45, 3), (64, 64, 2)):
        most = per_cu * 256
        for max_points, want in ((0, most), (1, 1), (1024, 1), (1025, 1), (4096, 1), (4097, 2), (3_000_000, min(733, most)), ((1 << 32) - 1, most)):
            g = d2pc.sectors_ground_geometry(d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b, max_points=max_points))
            n = n_a * n_b
            assert (g.n_cells, g.lds_bytes, g.blocks_per_cu, g.blocks) == (n, 20 * n, per_cu, want), (n_a, n_b, max_points)
            assert g.lds_bytes * g.blocks_per_cu <= 160 * 1024 and g.block_bytes == 20 * n + (4 if n % 2 else 0)
            assert g.device_bytes == g.blocks * g.block_bytes + 13 * n
    g = d2pc.sectors_ground_geometry(d2pc.sectors_ground_config_init(cell_size=0.3, quantum=0.01))
    assert F32(g.inv_c) == F32(1.0 / float(F32(0.3))) and F32(g.inv_q) == F32(1.0 / float(F32(0.01)))


def test_spread_of_std_against_float64():
    rng = np.random.default_rng(5)
    for q, s in [(0.002, 0.05), (1.0, 0.0), (1.0, 2.5), (0.001, 0.0315), (1.0, 65535.9)] + [
            (float(a), float(b)) for a, b in zip(rng.uniform(1e-4, 0.1, 200), rng.uniform(0.0, 2.0, 200))]:
        assert d2pc.sectors_ground_spread_of_std(q, s) == min(int(np.floor((np.float64(s) / np.float64(q)) ** 2)), 0xFFFFFFFE), (q, s)
    assert d2pc.sectors_ground_spread_of_std(0.002, 0.05) == 625
    assert d2pc.sectors_ground_spread_of_std(1.0, 65536.0) == 0xFFFFFFFE and d2pc.sectors_ground_spread_of_std(1.0, np.inf) == 0xFFFFFFFE
    for q, s in ((0.0, 1.0), (-1.0, 1.0), (np.nan, 1.0), (np.inf, 1.0), (1.0, np.nan), (1.0, -0.5)):
        assert d2pc.sectors_ground_spread_of_std(q, s) == 0, (q, s)


# ----------------------------------------------------------------------------------------- the reference against float64
def test_reference_binning_against_float64():
    """200,000 seeded points under a yaw / pitch / roll of 0.7 / 0.25 / -0.15 rad and a translation of tens of metres, on the
    default 16 x 16 grid of 0.5 m cells.  Points whose float64 va or vb lies within 1e-3 of an integer are left out (at most
    1 % may be; a numpy prototype left out 0.4 %); among the rest the gate and the cell agree exactly and k is within 1 of the
    float64 height (the prototype: |k - v_exact| <= 0.51)."""
    cfg = d2pc.sectors_ground_config_init()
    ref = gref.SectorsGroundRef(cfg, d2pc.sectors_ground_geometry(cfg))
    rng = np.random.default_rng(20)
    R64 = gref.rotation(0.7, 0.25, -0.15)
    t64 = np.array([31.5, -47.25, 22.0])
    origin = np.array([28.0, -51.0, 21.0], dtype=F32)
    world = np.stack([rng.uniform(27.0, 37.0, 200_000), rng.uniform(-52.0, -42.0, 200_000), rng.uniform(20.5, 21.5, 200_000)], axis=1)
    xyz = ((world - t64) @ R64).astype(F32)                      # R^T (w - t): the camera-frame records
    step = gref.step_words(R64, t64, origin)
    part, cell, k = ref.bin(xyz, step)
    R, t = step[:9].view(F32).astype(np.float64).reshape(3, 3), step[9:12].view(F32).astype(np.float64)
    w = xyz.astype(np.float64) @ R.T + t
    va, vb = (w[:, 0] - float(origin[0])) / float(F32(0.5)), (w[:, 1] - float(origin[1])) / float(F32(0.5))
    v = (w[:, 2] - float(origin[2])) / float(F32(0.002))
    keep = (np.abs(va - np.rint(va)) > 1e-3) & (np.abs(vb - np.rint(vb)) > 1e-3) & (np.abs(np.abs(v) - 32767.0) > 1.0)
    left_out = 1.0 - keep.mean()
    print("left out %.2f %%" % (100 * left_out))
    assert left_out <= 0.01
    part64 = (va >= 0) & (va < 16) & (vb >= 0) & (vb < 16) & (np.abs(v) <= 32767)
    assert 0.3 < part64.mean() < 0.9, "the gate must cut on every side"
    assert np.count_nonzero(part[keep] != part64[keep]) == 0
    both = keep & part64
    cell64 = np.floor(vb).astype(np.int64) * 16 + np.floor(va).astype(np.int64)
    assert np.count_nonzero(cell[both] != cell64[both]) == 0
    assert np.abs(k[both] - np.rint(v[both])).max() <= 1
    print("max |k - v_exact| = %.3f" % np.abs(k[both] - v[both]).max())
    assert len(np.unique(cell[both])) == 256 and np.abs(k[both]).max() > 200


# ---------------------------------------------------------------------------------------------- the two forms of S
def check_wrapped(ks):
    ks = np.asarray(ks, dtype=np.int64)
    count, total, total2 = len(ks), int(ks.sum()), int((ks * ks).sum())
    m = total // count                                              # Python's floor division
    direct = int(((ks - m) ** 2).sum())
    assert gref.wrapped_spread_sum(count, total, total2, m) == direct and direct < 1 << 64
    assert direct // count <= 65534 ** 2
    return m, direct // count


def test_wrapped_formula_for_S_equals_the_direct_sum():
    rng = np.random.default_rng(11)
    cfg = d2pc.sectors_ground_config_init(n_a=40, n_b=25)
    ref = gref.SectorsGroundRef(cfg, d2pc.sectors_ground_geometry(cfg))
    cell = rng.integers(0, 1000, 60_000)
    k = np.where(rng.random(60_000) < 0.3, rng.integers(-32767, 32768, 60_000), rng.integers(-40, 40, 60_000) + 20_000 * rng.integers(-1, 2, 60_000)[cell % 3])
    out = ref.cells(cell, k)
    assert (out["count"] > 0).all()
    for c in range(1000):
        m, spread = check_wrapped(k[cell == c])
        assert (out["mean_q"][c], out["spread_q2"][c]) == (m, spread), c
    assert (out["mean_q"] < 0).any() and (out["mean_q"] > 0).any()
    m, spread = check_wrapped([-32767, 32767])
    assert (m, spread) == (0, 32767 ** 2)
    m, spread = check_wrapped([-32767, -32767, 32767])
    assert m == -10923 and spread == ((32767 - 10923) ** 2 * 2 + (32767 + 10923) ** 2) // 3, "floor division towards -inf"
    m, spread = check_wrapped(np.full(1 << 20, 32767))
    assert (m, spread) == (32767, 0) and (1 << 20) * 32767 ** 2 > 1 << 49
    m, spread = check_wrapped(np.concatenate([np.full(1 << 19, 32767), np.full(1 << 19, -32767)]))
    assert (m, spread) == (0, 32767 ** 2)
    # an empty cell among full ones
    out = ref.cells(np.array([0, 0, 2]), np.array([5, 8, -3]))
    assert out["count"][:3].tolist() == [2, 0, 1] and out["mean_q"][:3].tolist() == [6, -(1 << 31), -3] and out["spread_q2"][:3].tolist() == [2, 0xFFFFFFFF, 0]
    assert out["sum"][:3].tolist() == [13, 0, -3] and out["sum2"][:3].tolist() == [89, 0, 9] and out["flat"][:3].tolist() == [0, 0, 0]


# ------------------------------------------------------------------------------------------------------ the sites
def test_sites_direct_window_against_brute_force():
    """1,000 seeded small grids: W = 0 .. 3 (W = 0 and windows wider than the grid included: then there are no sites)."""
    rng = np.random.default_rng(2)
    some = wider = 0
    for it in range(1000):
        n_a, n_b, W = int(rng.integers(2, 9)), int(rng.integers(2, 9)), int(rng.integers(0, 4)) if it % 10 else 8
        cfg = d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b, window=W, max_step_q=int(rng.integers(0, 4)))
        ref = gref.SectorsGroundRef(cfg, d2pc.sectors_ground_geometry(cfg))
        n = n_a * n_b
        mean = rng.integers(-3, 4, n).astype(np.int32) if it % 3 else np.zeros(n, dtype=np.int32)
        flat = (rng.random(n) < (0.95 if it % 2 else 0.7)).astype(np.uint8)
        allowed = (rng.random(n) < 0.8).astype(np.uint8) if it % 4 == 0 else None
        got = ref.sites(mean, flat, allowed)
        want = gref.brute_sites(n_a, n_b, W, ref.max_step_q, mean, flat, allowed)
        assert np.array_equal(got, want), (it, n_a, n_b, W)
        some += int(got.sum())
        if 2 * W + 1 > min(n_a, n_b):
            wider += 1
            assert not got.any()
        if W == 0 and allowed is None:
            assert np.array_equal(got, flat)
    assert some > 1000 and wider > 100


def test_candidates_order_ties_and_tail():
    cfg = d2pc.sectors_ground_config_init(n_a=6, n_b=5, w_dist=3, w_rough=2, rough_cap=10)
    ref = gref.SectorsGroundRef(cfg, d2pc.sectors_ground_geometry(cfg))
    site = np.ones(30, dtype=np.uint8)
    site[[0, 7]] = 0
    spread = np.arange(30) % 4 * 5                                    # 0, 5, 10, 15 (capped to 10)
    got = ref.candidates(site, spread, 2, 1, 32)
    n_sites = int(site.sum())
    assert np.all(np.diff(got[:n_sites].astype(np.float64)) > 0) and np.all(got[n_sites:] == gref.NO_CANDIDATE)
    cells = (got[:n_sites] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert sorted(cells.tolist()) == [c for c in range(30) if site[c]]
    for key in got[:n_sites]:
        c = int(key) & 0xFFFFFFFF
        i, j = c % 6, c // 6
        assert int(key) >> 32 == 3 * ((i - 2) ** 2 + (j - 1) ** 2) + 2 * min(int(spread[c]), 10)
    assert got[0] == (2 * 0 << 32) | 8                               # the goal cell itself: spread 0
    # ties go to the smaller cell; the goal switched off by either index
    for goal in ((6, 1), (2, 5), (0xFFFFFFFF, 0xFFFFFFFF)):
        flat_cost = ref.candidates(site, np.zeros(30, dtype=np.int64), goal[0], goal[1], 5)
        assert flat_cost.tolist() == [1, 2, 3, 4, 5]
    assert ref.candidates(np.zeros(30, dtype=np.uint8), spread, 2, 1, 3).tolist() == [gref.NO_CANDIDATE] * 3
    assert ref.candidates(site, spread, 2, 1, 1).tolist() == [8]
    big = d2pc.sectors_ground_config_init(n_a=64, n_b=64, w_dist=4095, w_rough=4095, rough_cap=65535)
    ref = gref.SectorsGroundRef(big, d2pc.sectors_ground_geometry(big))
    assert int(ref.cost(np.full(4096, 0xFFFFFFFE, dtype=np.int64), 0, 0).max()) == 4095 * (2 * 63 * 63 + 65535) < 0xFFFFFFFF
