"""The memory of the obstacle sectors (d2pc_sectors_memory_*) without a GPU: the header, the binding and the exports agree
on the new symbols; the struct sizes; the refusals of create and of d2pc_sectors_memory_desc_check through the library and
again through a stand-alone program under sanitizers; the coverage against numpy; tests/sectors_memory_ref.py (the
specification in float32) against float64 binning after a rigid motion.  tests/README_sectors_memory.md has the map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_elev_ref
import sectors_memory_ref as mref
import sectors_ref
from disparity_to_point_cloud_amd import sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, CAPACITY, NO_DEVICE = 1, 3, 4, 5
F32 = np.float32
MEMORY_SYMBOLS = ["d2pc_sectors_memory_coverage", "d2pc_sectors_memory_create", "d2pc_sectors_memory_desc_check",
                  "d2pc_sectors_memory_desc_init", "d2pc_sectors_memory_destroy", "d2pc_sectors_memory_last_error",
                  "d2pc_sectors_memory_reset_device", "d2pc_sectors_memory_update_device"]


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_hold_the_memory_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d2pc_sectors.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))
    assert sorted(n for n in declared if "_memory_" in n) == MEMORY_SYMBOLS
    assert sorted(n for n in sectors.SECTORS_SYMBOLS if "_memory_" in n) == MEMORY_SYMBOLS
    lib = d2pc.load_sectors_library()
    out = subprocess.run(["nm", "-D", "--defined-only", d2pc.sectors_library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    for name in MEMORY_SYMBOLS:
        assert hasattr(lib, name) and name in exported, name
    assert d2pc.SectorsMemory is sectors.SectorsMemory


def test_struct_sizes(tmp_path):
    """The new structs are pinned, the old ones are what they were, and the C compiler agrees with the binding."""
    assert ctypes.sizeof(d2pc.SectorsConfig) == 80 and ctypes.sizeof(d2pc.SectorsDesc) == 80 and ctypes.sizeof(d2pc.SectorsGeometry) == 72
    sizes = dict(d2pc_sectors_memory_config=(d2pc.SectorsMemoryConfig, 16), d2pc_sectors_memory_step=(d2pc.SectorsMemoryStep, 64),
                 d2pc_sectors_fov=(d2pc.SectorsFov, 40), d2pc_sectors_memory_desc=(d2pc.SectorsMemoryDesc, 104))
    for name, (cls, size) in sizes.items():
        assert ctypes.sizeof(cls) == size, name
    src = tmp_path / "sizes.c"
    src.write_text('#include "d2pc_sectors.h"\n' + "".join(
        "typedef char size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (n, n, s) for n, (_, s) in sizes.items()) +
        "typedef char size_of_config[sizeof(d2pc_sectors_config) == 80 && sizeof(d2pc_sectors_desc) == 80 ? 1 : -1];\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "sizes.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    d = d2pc.sectors_memory_desc_init()
    assert (d.struct_size, d.point_step, d.n_clouds, d.cloud_points, d.points_frame_stride_points) == (104, 16, 1, 0, 0)
    assert all(getattr(d, k) is None for k in ("points", "count", "nearest", "step", "covered", "range", "distance_cm", "age", "records"))
    m = d2pc.sectors_memory_config(1234)
    assert (m.struct_size, m.max_age, list(m.reserved)) == (16, 1234, [0, 0])
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_memory_desc_init(None)     # tolerated
    assert lib.d2pc_sectors_memory_last_error(None) == b"null session"
    assert lib.d2pc_sectors_memory_destroy(None) == INVALID_ARG and lib.d2pc_sectors_memory_reset_device(None, None) == INVALID_ARG
    assert lib.d2pc_sectors_memory_update_device(None, ctypes.byref(d), None) == INVALID_ARG
    w = d2pc.sectors_memory_step(np.arange(9).reshape(3, 3), [10, 11, 12], 77)
    assert w.dtype == np.uint32 and w[:12].view(F32).tolist() == list(range(9)) + [10, 11, 12] and w[12:].tolist() == [77, 0, 0, 0]
    assert np.array_equal(w, mref.step_words(np.arange(9), [10, 11, 12], 77))


# ------------------------------------------------------------------------------------------------------ refusals
def test_create_refusals_and_no_device():
    lib = d2pc.load_sectors_library()
    h, g = ctypes.c_void_p(), d2pc.SectorsGeometry()
    no_gpu = d2pc.device_count() == 0

    def status(max_age=1000, struct_size=16, **kw):
        cfg = d2pc.sectors_config_init(**kw)
        m = d2pc.sectors_memory_config(max_age)
        m.struct_size = struct_size
        st = lib.d2pc_sectors_memory_create(ctypes.byref(cfg), ctypes.byref(m), ctypes.byref(h))
        if h:
            lib.d2pc_sectors_memory_destroy(h)
        grid = lib.d2pc_sectors_geometry(ctypes.byref(cfg), ctypes.byref(g))
        if grid:
            assert st == grid, "create refuses the grid as d2pc_sectors_create does"
        return st

    ok = NO_DEVICE if no_gpu else 0
    good, m = d2pc.sectors_config_init(), d2pc.sectors_memory_config(5)
    assert lib.d2pc_sectors_memory_create(ctypes.byref(good), ctypes.byref(m), None) == INVALID_ARG
    assert lib.d2pc_sectors_memory_create(None, ctypes.byref(m), ctypes.byref(h)) == INVALID_ARG
    assert lib.d2pc_sectors_memory_create(ctypes.byref(good), None, ctypes.byref(h)) == INVALID_ARG and not h
    assert status() == ok and status(max_age=0) == ok and status(max_age=0xFFFFFFFE) == ok
    assert status(max_age=0xFFFFFFFF) == INVALID_ARG and status(struct_size=12) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for kw in (dict(n_sectors=71), dict(axes=(1, 1, 2)), dict(r_min=-1.0), dict(min_count=0), dict(layer_kind=2), dict(azimuth0=np.inf)):
        assert status(**kw) == INVALID_ARG, kw
    half_pi = float(F32(np.pi / 2))
    for kw in (dict(n_layers=17), dict(n_layers=2), dict(layer_kind=1, n_layers=65, u_min=-1.0, u_max=1.0),
               dict(layer_kind=1, n_sectors=92, n_layers=64, u_min=-1.0, u_max=1.0), dict(layer_kind=1, u_min=-2.0, u_max=1.0),
               dict(n_layers=2, max_age=0xFFFFFFFF)):      # the grid's refusal comes first
        assert status(**kw) == BAD_SIZE, kw
    assert status(n_sectors=360, n_layers=16, u_min=-1.0, u_max=1.0) == ok
    assert status(layer_kind=1, n_sectors=90, n_layers=64, u_min=-half_pi, u_max=half_pi) == ok
    if no_gpu:
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.SectorsMemory(good)
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_config_init(device_id=1 << 20)
    assert lib.d2pc_sectors_memory_create(ctypes.byref(bad), ctypes.byref(m), ctypes.byref(h)) == NO_DEVICE


def test_desc_refusals_without_a_device():
    """d2pc_sectors_memory_desc_check is d2pc_sectors_memory_update_device's own check (csrc/d2pc_sectors_memory_plan.hpp);
    the pointers are numbers here, nothing is dereferenced."""
    cfg, mcfg = d2pc.sectors_config_init(), d2pc.sectors_memory_config(5000)    # 72 cells
    P, CN, NR, ST, CV = 0x10000000, 0x20000000, 0x20001000, 0x20002000, 0x20003000
    RG, CM, AG, RC = 0x30000000, 0x30001000, 0x30002000, 0x30003000
    n = 1000
    good = dict(points=P, cloud_points=n, count=CN, nearest=NR, step=ST, covered=CV, range=RG, distance_cm=CM, age=AG, records=RC)
    outs = ("range", "distance_cm", "age", "records")

    def status(cfg=cfg, mcfg=mcfg, **kw):
        return d2pc.sectors_memory_desc_check(cfg, mcfg, d2pc.sectors_memory_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    desc = d2pc.sectors_memory_desc_init(**good)
    assert status() == 0 and status(point_step=32) == 0 and status(covered=None) == 0
    assert lib.d2pc_sectors_memory_desc_check(ctypes.byref(cfg), ctypes.byref(mcfg), None) == INVALID_ARG
    assert lib.d2pc_sectors_memory_desc_check(None, ctypes.byref(mcfg), ctypes.byref(desc)) == INVALID_ARG
    assert lib.d2pc_sectors_memory_desc_check(ctypes.byref(cfg), None, ctypes.byref(desc)) == INVALID_ARG
    assert status(cfg=d2pc.sectors_config_init(n_sectors=7)) == INVALID_ARG and status(cfg=d2pc.sectors_config_init(n_layers=17)) == BAD_SIZE
    assert status(mcfg=d2pc.sectors_memory_config(0xFFFFFFFF)) == INVALID_ARG
    assert status(struct_size=96) == INVALID_ARG
    for step in (0, 8, 12, 24, 48, 64, -16):
        assert status(point_step=step) == INVALID_ARG, step
    for k in (0, -1, 65536):
        assert status(n_clouds=k, points_frame_stride_points=n) == INVALID_ARG, k
    for k in ("points", "count", "nearest", "step"):
        assert status(**{k: None}) == INVALID_ARG, k
    assert status(**{k: None for k in outs}) == INVALID_ARG
    for only in outs:
        assert status(**{k: (good[k] if k == only else None) for k in outs}) == 0, only
    # alignment to type; points and records to 16 bytes
    assert status(points=P + 8) == INVALID_ARG and status(points=P + 16) == 0
    assert status(records=RC + 8) == INVALID_ARG and status(records=RC + 16) == 0
    for k, off in (("count", 2), ("nearest", 1), ("step", 2), ("range", 2), ("age", 2), ("distance_cm", 1)):
        assert status(**{k: good[k] + off}) == INVALID_ARG, k
    assert status(distance_cm=CM + 2) == 0 and status(step=ST + 4) == 0 and status(covered=CV + 1) == 0
    # sizes: the position bound as the sectors refuse it
    big = 1 << 44
    assert status(cloud_points=0) == BAD_SIZE and status(points=big, cloud_points=1 << 32) == BAD_SIZE
    assert status(points=big, cloud_points=(1 << 32) - 1) == 0
    assert status(n_clouds=3, points_frame_stride_points=n - 1) == BAD_SIZE and status(n_clouds=3, points_frame_stride_points=n) == 0
    assert status(n_clouds=1, points_frame_stride_points=0) == 0
    assert status(points=big, n_clouds=2, cloud_points=1 << 30, points_frame_stride_points=(3 << 30) - 1) == 0
    assert status(points=big, n_clouds=2, cloud_points=1 << 30, points_frame_stride_points=3 << 30) == BAD_SIZE
    assert status(points=big, n_clouds=65535, cloud_points=1, points_frame_stride_points=65539) == BAD_SIZE
    assert status(points=big, n_clouds=65535, cloud_points=1, points_frame_stride_points=65538) == 0
    assert status(points=big, n_clouds=2, cloud_points=5, points_frame_stride_points=1 << 63) == BAD_SIZE
    # overlaps: an output over the last byte of every input, and of another output
    assert status(range=P) == INVALID_ARG and status(age=P + 16 * n - 4) == INVALID_ARG and status(age=P + 16 * n) == 0
    assert status(point_step=32, age=P + 32 * n - 4) == INVALID_ARG
    assert status(n_clouds=3, points_frame_stride_points=n + 7, age=P + 16 * (2 * (n + 7) + n) - 4) == INVALID_ARG
    assert status(n_clouds=3, points_frame_stride_points=n + 7, age=P + 16 * (2 * (n + 7) + n)) == 0
    for base, size in ((CN, 288), (NR, 288), (ST, 64), (CV, 72)):
        assert status(distance_cm=base + size - 2) == INVALID_ARG and status(distance_cm=base + size) == 0, hex(base)
        assert status(records=base - 1152 + 16) == INVALID_ARG and status(records=base - 1152) == 0, hex(base)
    assert status(covered=None, distance_cm=CV + 70) == 0
    assert status(age=RG + 284) == INVALID_ARG and status(age=RG + 288) == 0
    assert status(range=CM + 140) == INVALID_ARG and status(range=CM + 144) == 0
    assert status(records=AG + 272) == INVALID_ARG and status(records=AG + 288) == 0
    assert status(age=RC + 1148) == INVALID_ARG and status(age=RC + 1152) == 0
    # the extents follow the session's cells
    wide = d2pc.sectors_config_init(n_sectors=360, n_layers=16, u_min=0.0, u_max=4.0)
    far = dict(nearest=0x21000000, step=0x22000000, covered=0x23000000, distance_cm=None)
    assert status(cfg=wide, age=RG + 4 * 5760 - 4, records=None, **far) == INVALID_ARG
    assert status(cfg=wide, age=RG + 4 * 5760, records=None, **far) == 0
    only = dict(far, range=None, age=None)
    assert status(cfg=wide, records=CN + 4 * 5760 - 16, **only) == INVALID_ARG and status(cfg=wide, records=CN + 4 * 5760, **only) == 0
    assert status(cfg=wide, records=0x23000000 + 5760 - 16, **only) == INVALID_ARG and status(cfg=wide, records=0x23000000 + 5760, **only) == 0
    assert status(cfg=wide, records=0x23000000 - 16 * 5760 + 16, **only) == INVALID_ARG and status(cfg=wide, records=0x23000000 - 16 * 5760, **only) == 0


def test_memory_plan_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/sectors_memory_plan_main.cpp, a stand-alone program over csrc/d2pc_sectors_memory_plan.hpp (host code,
    nothing loaded into Python): both refusal matrices, the position bound and the coverage, with -fsanitize=address,undefined."""
    exe = tmp_path / "sectors_memory_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sectors_memory_plan_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------ the coverage
def _coverage_numpy(cfg, fovs):
    """-> (covered uint8, the smallest distance of a centre to a field of view's edge in radians)."""
    n, layers = cfg.n_sectors, cfg.n_layers
    az = cfg.azimuth0 + 2 * np.pi * (np.arange(n) + 0.5) / n
    elevation = cfg.layer_kind == d2pc.LAYERS_ELEVATION
    el = np.zeros(layers)
    if elevation:
        e = sectors_elev_ref.boundary_elevations(cfg.u_min, cfg.u_max, layers)
        el = (e[:-1] + e[1:]) / 2
    cov, edge = np.zeros((layers, n), dtype=bool), np.inf
    for yaw, pitch, h_fov, v_fov, margin in fovs:
        x = az - yaw
        da = np.abs(x - 2 * np.pi * np.round(x / (2 * np.pi)))
        inside = np.broadcast_to(da <= h_fov / 2 - margin, (layers, n))
        edge = min(edge, np.abs(da - (h_fov / 2 - margin)).min())
        if elevation:
            de = np.abs(el - pitch)
            inside = inside & (de <= v_fov / 2 - margin)[:, None]
            edge = min(edge, np.abs(de - (v_fov / 2 - margin)).min())
        cov |= inside
    return cov.reshape(-1).astype(np.uint8), edge


@pytest.mark.parametrize("grid", [dict(), dict(n_sectors=12, n_layers=4, u_min=-2.0, u_max=2.0), dict(n_sectors=360, azimuth0=0.3),
                                  dict(n_sectors=60, n_layers=30, layer_kind=1, u_min=-1.5707964, u_max=1.5707964, azimuth0=-np.pi / 60),
                                  dict(n_sectors=8, n_layers=5, layer_kind=1, u_min=-0.4, u_max=0.9)],
                         ids=["72x1", "12x4", "360x1", "60x30e", "8x5e"])
def test_coverage_against_numpy(grid):
    cfg = d2pc.sectors_config_init(**grid)
    cases = [[(0.0, 0.0, np.deg2rad(87.0), np.deg2rad(58.0), 0.0)],
             [(0.0, 0.1, np.deg2rad(87.0), np.deg2rad(58.0), np.deg2rad(4.1))],
             [(3.1, -0.2, 1.234, 0.777, 0.01), (-1.7 - 4 * np.pi, 0.3, 0.9, 2.0, 0.0)],     # across +-pi; a yaw turns away
             [(1.0, 0.0, 7.0, 4.0, 0.0)],                                                   # wider than a turn: everything
             [(1.0, 0.0, 0.5, 0.5, 0.3)]]                                                   # the margin eats it: nothing
    for fovs in cases:
        want, edge = _coverage_numpy(cfg, fovs)
        assert edge > 1e-9, "a cell centre lies on a field of view's edge: choose another case"
        got = d2pc.sectors_memory_coverage(cfg, fovs)
        assert got.dtype == np.uint8 and np.array_equal(got, want), (grid, fovs)
    assert _coverage_numpy(cfg, cases[3])[0].all() and not _coverage_numpy(cfg, cases[4])[0].any()
    assert 0 < _coverage_numpy(cfg, cases[0])[0].sum() < cfg.n_sectors * cfg.n_layers
    assert not d2pc.sectors_memory_coverage(cfg, []).any()


def test_coverage_refusals():
    lib = d2pc.load_sectors_library()
    cfg = d2pc.sectors_config_init()
    fov = d2pc.SectorsFov(0.0, 0.0, 1.0, 1.0, 0.0)
    buf = np.full(80, 9, dtype=np.uint8)
    p = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), ctypes.byref(fov), 1, p, 71) == -CAPACITY
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), ctypes.byref(fov), 1, None, 72) == -INVALID_ARG
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), None, 1, p, 72) == -INVALID_ARG
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), ctypes.byref(fov), -1, p, 72) == -INVALID_ARG
    assert lib.d2pc_sectors_memory_coverage(None, ctypes.byref(fov), 1, p, 72) == -INVALID_ARG
    cfg.n_layers = 17
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), ctypes.byref(fov), 1, p, 80) == -BAD_SIZE
    assert np.all(buf == 9), "a refused call wrote"
    cfg.n_layers = 1
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), ctypes.byref(fov), 1, p, 72) == 72 and np.all(buf[72:] == 9)
    assert lib.d2pc_sectors_memory_coverage(ctypes.byref(cfg), None, 0, p, 72) == 72 and not buf[:72].any()


# -------------------------------------------------------------------------------- the reference against float64 binning
def grid_ref(cfg):
    table, geo = d2pc.sectors_table(cfg), d2pc.sectors_geometry(cfg)
    if cfg.layer_kind == d2pc.LAYERS_ELEVATION:
        return sectors_elev_ref.SectorsElevRef(cfg, table, geo, d2pc.sectors_elevation_table(cfg))
    return sectors_ref.SectorsRef(cfg, table, geo)


def _float64_cells(cfg, p):
    """float64 binning of points p (n, 3) in a body frame (axes 1, 2, 3) -> (takes part, cell, near a boundary)."""
    n, layers = cfg.n_sectors, cfg.n_layers
    f, l, u = p[:, 0], p[:, 1], p[:, 2]
    a = np.mod(np.arctan2(l, f) - cfg.azimuth0, 2 * np.pi) / (2 * np.pi / n)
    sector = np.minimum(a.astype(np.int64), n - 1)
    near = np.abs(a - np.round(a)) * (2 * np.pi / n) < 1e-4
    if cfg.layer_kind == d2pc.LAYERS_ELEVATION:
        part, layer, off = sectors_elev_ref.atan2_layer(f, l, u, cfg.u_min, cfg.u_max, layers)
        near |= off < 1e-4
    else:
        lo, hi = float(F32(cfg.u_min)), float(F32(cfg.u_max))
        part = (u >= lo) & (u < hi)
        s = (u - lo) * (layers / (hi - lo)) if layers > 1 else np.zeros(len(u))
        layer = np.clip(np.floor(s), 0, layers - 1).astype(np.int64)
        edges = np.array([lo, hi]) if layers == 1 else lo + (hi - lo) * np.arange(layers + 1) / layers
        near |= np.abs(u[:, None] - edges[None, :]).min(axis=1) < 1e-4         # a slab's face, 1e-4 of the cloud's unit
    return part, layer * n + sector, near


MOTION_GRIDS = [dict(n_sectors=72), dict(n_sectors=12, n_layers=4, u_min=-9.0, u_max=9.0),
                dict(n_sectors=360, n_layers=16, u_min=-12.0, u_max=12.0),
                dict(n_sectors=60, n_layers=30, layer_kind=1, u_min=-1.5707964, u_max=1.5707964, azimuth0=-np.pi / 60)]


@pytest.mark.parametrize("grid", MOTION_GRIDS, ids=["72x1", "12x4", "360x16", "60x30e"])
def test_reference_agrees_with_float64_binning_after_a_rigid_motion(grid):
    """4,000 Gaussian points seen once; then the vehicle yaws 37 degrees, pitches a little, moves and climbs, and sees nothing.
    Identity first: the second call's range is the first's, bit for bit, and every age is dt.  Then every cell the
    reference keeps holds a point that float64 binning of R^T (w - t) puts into that very cell, every remembered point
    that float64 keeps finds its cell occupied by a point at most as far, and the ranges agree to 1e-6 relative: d, the
    five roundings of a rotated coordinate, r2 / d2 and the square root each move the range by at most 2^-24 of it or
    so, a dozen of them 7e-7 (the figure is printed).  Points within 1e-4 rad (or 1e-4 units of a slab's face) of a
    boundary are left out; they are at most 2 % of the remembered points."""
    cfg = d2pc.sectors_config_init(axes=(1, 2, 3), r_min=0.0, **grid)
    ref = grid_ref(cfg)
    xyz = (np.random.default_rng(cfg.n_sectors).normal(size=(4000, 3)) * 6.0).astype(F32)
    words = np.zeros((4000, 4), dtype=np.uint32)
    words[:, :3] = xyz.view(np.uint32)
    g = ref.grid(xyz, np.arange(4000))
    none = np.zeros(ref.n_cells, dtype=np.uint32), np.full(ref.n_cells, 0xFFFFFFFF, dtype=np.uint32)
    eye, zero = np.eye(3), np.zeros(3)
    mem = mref.SectorsMemoryRef(ref, max_age=10_000)
    first = mem.update(words, g["count"], g["nearest"], 4000, eye, zero, 0)
    assert first["range"].tobytes() == g["range"].tobytes() and np.array_equal(first["age"] == 0, g["count"] > 0)
    again = mem.update(words, *none, 4000, eye, zero, 33)
    assert again["range"].tobytes() == first["range"].tobytes()
    assert np.array_equal(again["records"][:, :3], first["records"][:, :3])
    assert np.all(again["age"][g["count"] > 0] == 33) and np.all(again["age"][g["count"] == 0] == 0xFFFFFFFF)
    # the motion
    R = mref.rotation(np.deg2rad(37.0), 0.02, -0.015).astype(F32)
    t = np.array([1.25, -0.75, 0.4], dtype=F32)
    old = again["records"]
    had = np.flatnonzero(old[:, 3] != 0xFFFFFFFF)
    moved = mem.update(words, *none, 4000, R, t, 10)
    p64 = (old[had, :3].copy().view(F32).astype(np.float64) - t.astype(np.float64)) @ R.astype(np.float64)   # rows of R^T (w - t)
    part, cell, near = _float64_cells(cfg, p64)
    k64 = np.sqrt((p64 ** 2).sum(axis=1) if cfg.layer_kind else (p64[:, :2] ** 2).sum(axis=1))
    share = near.mean()
    print("%d remembered, %.2f %% left out" % (len(had), 100 * share))
    assert share <= 0.02
    # every kept cell: float64 puts the record it holds into that cell
    kept = np.flatnonzero(moved["age"] != 0xFFFFFFFF)
    assert np.all(moved["age"][kept] == 43)
    where = {old[i, :3].tobytes(): j for j, i in enumerate(had)}
    agree = worst = 0
    for c in kept:
        j = where[moved["records"][c, :3].tobytes()]
        if near[j]:
            continue
        assert part[j] and cell[j] == c, "cell %d holds a point float64 puts into %s" % (c, cell[j] if part[j] else "no cell")
        worst = max(worst, abs(float(moved["range"][c]) / k64[j] - 1))
        agree += 1
    # every remembered point float64 keeps: its cell is occupied, by a point at most as far
    for j in np.flatnonzero(part & ~near):
        assert moved["age"][cell[j]] != 0xFFFFFFFF and float(moved["range"][cell[j]]) <= k64[j] * (1 + 1e-6)
    print("%d / %d kept cells agree, ranges within %.2g relative" % (agree, agree, worst))
    assert agree > len(kept) * 0.9 and worst <= 1e-6
