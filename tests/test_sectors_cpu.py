"""The obstacle sectors without a GPU: the header, the binding and the exports of libd2pc_sectors.so agree; the boundary
table against numpy; tests/sectors_ref.py (the specification in float32) against float64 atan2 binning; the defaults,
the geometry and every refusal that needs no device.  tests/README_sectors.md has the map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ref
from disparity_to_point_cloud_amd import capi, sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, CAPACITY, NO_DEVICE = 1, 3, 4, 5
OFFSETS = lambda n: (0.0, -np.pi / n, 0.3)  # noqa: E731


def _header_functions(name):
    src = open(os.path.join(ROOT, "include", name)).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))


def _exports(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return sorted({ln.split()[-1] for ln in out.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in ("T", "W")
                   and ln.split()[-1].startswith("d2pc_")})


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_agree():
    declared = _header_functions("d2pc_sectors.h")
    assert len(declared) >= 9 and all(n.startswith("d2pc_sectors_") for n in declared)
    assert sorted(sectors.SECTORS_SYMBOLS) == declared, "python binding and d2pc_sectors.h disagree"
    lib = d2pc.load_sectors_library()
    for name in declared:
        assert hasattr(lib, name), f"libd2pc_sectors.so does not export {name}"
    assert _exports(d2pc.sectors_library_path()) == declared, "the companion library exports another d2pc_* symbol"
    assert not [n for n in _exports(capi.library_path()) if n.startswith("d2pc_sectors")]
    assert not set(declared) & set(capi.ABI_SYMBOLS + capi.EXT_SYMBOLS)


def test_companion_library_links_the_hip_runtime_only():
    out = subprocess.run(["readelf", "-d", d2pc.sectors_library_path()], capture_output=True, text=True, check=True).stdout
    needed = re.findall(r"NEEDED.*\[(.+?)\]", out)
    assert any(n.startswith("libamdhip64") for n in needed) and not [n for n in needed if "d2pc" in n], needed


def test_header_is_plain_c99_and_cxx11(tmp_path):
    src = tmp_path / "hdr.c"
    src.write_text('#include "d2pc_sectors.h"\nint main(void) { d2pc_sectors_config c; d2pc_sectors_desc d; '
                   'd2pc_sectors_geometry_t g; (void)c; (void)d; (void)g; return D2PC_SECTORS_MAX_SECTORS == 360 ? 0 : 1; }\n')
    for cmd in (["gcc", "-std=c99"], ["g++", "-std=c++11", "-x", "c++"]):
        p = subprocess.run(cmd + ["-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                                  str(src), "-o", str(tmp_path / "hdr.o")], capture_output=True, text=True)
        assert p.returncode == 0, p.stderr


def test_plan_header_needs_no_hip(tmp_path):
    """csrc/d2pc_sectors_plan.hpp holds the refusals and the host arithmetic: plain g++ compiles and runs it."""
    src = tmp_path / "plan.cpp"
    src.write_text(
        '#include "d2pc_sectors_plan.hpp"\n#include <cmath>\nusing namespace d2pc::sectors;\n'
        'int main() { d2pc_sectors_config c; memset(&c, 0, sizeof c); c.struct_size = sizeof c; c.n_sectors = 72; c.n_layers = 1;\n'
        '  c.r_min = 0.5f; c.r_max = INFINITY; c.u_min = -INFINITY; c.u_max = INFINITY; c.axes[0] = 3; c.axes[1] = -1; c.axes[2] = -2;\n'
        '  c.min_count = 1; Plan p; char msg[128];\n'
        '  if (make_plan(&c, &p, msg, sizeof msg) != D2PC_OK || p.n_cells != 72 || p.rmin2 != 0.25f || p.lds_bytes != 72 * 12 + 36 * 8) return 1;\n'
        '  c.n_sectors = 71; if (make_plan(&c, &p, msg, sizeof msg) != D2PC_ERR_INVALID_ARG || !msg[0]) return 2;\n'
        '  return 0; }\n')
    exe = tmp_path / "plan"
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I",
                        os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc"), str(src), "-o", str(exe)],
                       capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert subprocess.run([str(exe)]).returncode == 0


# ------------------------------------------------------------------------------------------------------- the table
def _ulp_apart(a, b):
    ia, ib = (np.asarray(v, dtype=np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7FFFFFFF), i) for i in (ia, ib))
    return np.abs(ia - ib)


@pytest.mark.parametrize("n", [2, 4, 72, 360])
def test_table_against_numpy(n):
    for az in OFFSETS(n) + (-7.25, 100.0):
        c, s = d2pc.sectors_table(d2pc.sectors_config_init(n_sectors=n, azimuth0=az))
        assert c.dtype == s.dtype == np.float32 and len(c) == len(s) == n // 2
        ang = az + 2 * np.pi * np.arange(n // 2) / n
        assert _ulp_apart(c, np.cos(ang).astype(np.float32)).max() <= 1 and _ulp_apart(s, np.sin(ang).astype(np.float32)).max() <= 1
    c, s = d2pc.sectors_table(d2pc.sectors_config_init(n_sectors=n, azimuth0=0.0))
    assert c[0].tobytes() == np.float32(1.0).tobytes() and s[0].tobytes() == np.float32(0.0).tobytes()
    lib = d2pc.load_sectors_library()
    cfg = d2pc.sectors_config_init(n_sectors=n)
    fp = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(400, dtype=np.float32)
    assert lib.d2pc_sectors_table(ctypes.byref(cfg), buf.ctypes.data_as(fp), buf[200:].ctypes.data_as(fp), n // 2 - 1) == -CAPACITY
    assert lib.d2pc_sectors_table(ctypes.byref(cfg), None, buf.ctypes.data_as(fp), 200) == -INVALID_ARG
    assert lib.d2pc_sectors_table(None, buf.ctypes.data_as(fp), buf[200:].ctypes.data_as(fp), 200) == -INVALID_ARG
    cfg.n_sectors = n + 1
    assert lib.d2pc_sectors_table(ctypes.byref(cfg), buf.ctypes.data_as(fp), buf[200:].ctypes.data_as(fp), 200) == -INVALID_ARG
    assert not buf.any(), "a refused call wrote the table"


# ------------------------------------------------------------------------------------- the reference against atan2
def _ref(cfg):
    return sectors_ref.SectorsRef(cfg, d2pc.sectors_table(cfg), d2pc.sectors_geometry(cfg))


@pytest.mark.parametrize("n", [2, 4, 72, 360])
def test_reference_agrees_with_float64_atan2(n):
    """Points in polar form at least 1e-4 rad from every boundary, ranges 1e-3 .. 1e4: none is excluded, all agree.
    (The float32 coordinates move a direction by 1e-7 rad at the most, the table's rounding a boundary as little.)"""
    rng = np.random.default_rng(n)
    m, width = 100_000, 2 * np.pi / n
    for az in OFFSETS(n):
        cfg = d2pc.sectors_config_init(n_sectors=n, azimuth0=az, r_min=0.0, axes=(1, 2, 3))
        k = rng.integers(0, n, size=m)
        theta = az + (k + rng.uniform(0, 1, size=m) * (1 - 2e-4 / width) + 1e-4 / width) * width
        r = 10.0 ** rng.uniform(-3, 4, size=m)
        xyz = np.stack([r * np.cos(theta), r * np.sin(theta), rng.normal(size=m)], axis=1).astype(np.float32)
        part, cell, _ = _ref(cfg).cells(xyz)
        assert part.all()
        assert np.array_equal(cell, k), (n, az)
        assert np.array_equal(sectors_ref.atan2_sector(xyz[:, 0], xyz[:, 1], n, az), k)
    # the axis picks: the optical frame's forward is z, left is -x, up is -y; clockwise numbering mirrors the sectors
    cfg = d2pc.sectors_config_init(n_sectors=n, azimuth0=0.3, r_min=0.0)
    opt = np.stack([-xyz[:, 1], -xyz[:, 2], xyz[:, 0]], axis=1)
    assert np.array_equal(_ref(cfg).cells(opt)[1], k)
    cw = d2pc.sectors_config_init(n_sectors=n, azimuth0=-0.3 - 2 * np.pi, r_min=0.0, axes=(1, -2, 3))
    got = _ref(cw).cells(xyz)[1]
    assert np.array_equal(got, sectors_ref.atan2_sector(xyz[:, 0], -xyz[:, 1], n, -0.3))


def test_reference_grid_on_a_hand_made_cloud():
    """Four points, by hand: the key's tie-break, min_count's mask, the cm forms."""
    cfg = d2pc.sectors_config_init(n_sectors=4, azimuth0=-np.pi / 4, r_min=0.0, axes=(1, 2, 3), min_count=2, no_obstacle_cm=901)
    xyz = np.array([[3, 0, 0], [3, 0, 5], [2.995, 0, 1], [0, 700, 0], [0, 0, 9], [np.nan, 1, 1]], dtype=np.float32)
    g = _ref(cfg).grid(xyz, np.array([7, 5, 9, 11, 12, 13]))
    assert g["count"].tolist() == [3, 1, 0, 0] and g["nearest"].tolist() == [9, 11, 0xFFFFFFFF, 0xFFFFFFFF]
    assert g["range"][0] == np.float32(2.995) and np.isinf(g["range"][1:]).all()
    assert g["distance_cm"].tolist() == [299, 901, 901, 901]
    cfg.min_count = 1
    g = _ref(cfg).grid(xyz[[0, 1, 3]], np.array([7, 5, 11]))
    assert g["nearest"].tolist() == [5, 11, 0xFFFFFFFF, 0xFFFFFFFF] and g["distance_cm"].tolist() == [300, 65534, 901, 901]


# ------------------------------------------------------------------------------------------- defaults and geometry
def test_defaults_and_struct_layouts():
    c = d2pc.sectors_config_init()
    assert ctypes.sizeof(d2pc.SectorsConfig) == 80 and ctypes.sizeof(d2pc.SectorsDesc) == 80 and ctypes.sizeof(d2pc.SectorsGeometry) == 72
    assert (c.struct_size, c.device_id, c.n_sectors, c.n_layers) == (80, 0, 72, 1)
    assert c.azimuth0 == -np.pi / 72 and c.r_min == np.float32(0.2) and c.r_max == np.inf and (c.u_min, c.u_max) == (-np.inf, np.inf)
    assert list(c.axes) == [3, -1, -2] and (c.min_count, c.no_obstacle_cm) == (1, 65535) and not any(c.reserved)
    d = d2pc.sectors_desc_init()
    assert (d.struct_size, d.point_step, d.n_clouds, d.cloud_points) == (80, 16, 1, 0)
    assert all(getattr(d, k) is None for k in ("points", "counts", "range", "count", "nearest", "distance_cm"))
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_config_init(None), lib.d2pc_sectors_desc_init(None)     # tolerated
    assert lib.d2pc_sectors_last_error(None) == b"null session" and lib.d2pc_sectors_blocks(None) == 0
    assert lib.d2pc_sectors_destroy(None) == INVALID_ARG and lib.d2pc_sectors_process_device(None, ctypes.byref(d), None) == INVALID_ARG


def test_geometry():
    g = d2pc.sectors_geometry(d2pc.sectors_config_init())
    assert (g.n_cells, g.table_entries, g.share_points, g.blocks_per_cu) == (72, 36, 1024, 4)
    assert g.rmin2 == np.float32(0.2) * np.float32(0.2) and g.rmax2 == np.inf and g.inv_h == 0.0
    assert g.lds_bytes == 72 * 12 + 36 * 8 and g.block_bytes == 72 * 12 and g.device_bytes == 1024 * 72 * 12 + 36 * 8
    g = d2pc.sectors_geometry(d2pc.sectors_config_init(n_sectors=360, n_layers=16, u_min=-1.5, u_max=2.5, r_min=0.3, r_max=25.0))
    assert (g.n_cells, g.table_entries, g.blocks_per_cu) == (5760, 180, 2) and g.lds_bytes == 5760 * 12 + 1440 <= 160 * 1024 // 2
    assert g.inv_h == np.float32(16 / 4.0) and g.rmin2 == np.float32(0.3) * np.float32(0.3) and g.rmax2 == 625.0
    g = d2pc.sectors_geometry(d2pc.sectors_config_init(n_layers=3, u_min=-0.1, u_max=0.6))
    assert g.inv_h == np.float32(3 / (float(np.float32(0.6)) - float(np.float32(-0.1))))


# ------------------------------------------------------------------------------------------------------ refusals
def test_config_refusals_and_no_device():
    lib = d2pc.load_sectors_library()
    g, h = d2pc.SectorsGeometry(), ctypes.c_void_p()

    def status(**kw):
        cfg = d2pc.sectors_config_init(**kw)
        st = lib.d2pc_sectors_geometry(ctypes.byref(cfg), ctypes.byref(g))
        assert lib.d2pc_sectors_create(ctypes.byref(cfg), ctypes.byref(h)) == (st or (NO_DEVICE if d2pc.device_count() == 0 else 0))
        if h:
            lib.d2pc_sectors_destroy(h)
        return st

    good = d2pc.sectors_config_init()
    assert lib.d2pc_sectors_geometry(None, ctypes.byref(g)) == INVALID_ARG and lib.d2pc_sectors_geometry(ctypes.byref(good), None) == INVALID_ARG
    assert lib.d2pc_sectors_create(ctypes.byref(good), None) == INVALID_ARG and lib.d2pc_sectors_create(None, ctypes.byref(h)) == INVALID_ARG
    assert status() == 0
    assert status(struct_size=76) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for axes in ((0, 1, 2), (1, 1, 2), (1, -1, 3), (1, 2, 4), (3, -1, 2 - (1 << 31)), (-(1 << 31), 1, 2)):
        assert status(axes=axes) == INVALID_ARG, axes
    for axes in ((1, 2, 3), (-3, 2, -1), (2, 3, 1)):
        assert status(axes=axes) == 0, axes
    for n in (0, 1, 3, 71, 361, 362, -2):
        assert status(n_sectors=n) == INVALID_ARG, n
    assert status(n_sectors=2) == 0 and status(n_sectors=360) == 0
    nan = float("nan")
    for kw in (dict(azimuth0=nan), dict(azimuth0=np.inf), dict(r_min=nan), dict(r_max=nan), dict(u_min=nan), dict(u_max=nan),
               dict(r_min=-0.5), dict(r_min=2.0, r_max=1.0), dict(r_min=np.inf, r_max=1e30), dict(u_min=1.0, u_max=0.5),
               dict(min_count=0), dict(min_count=-3), dict(no_obstacle_cm=65536)):
        assert status(**kw) == INVALID_ARG, kw
    assert status(r_min=0.0, r_max=0.0) == 0 and status(r_min=1.0, r_max=1.0) == 0 and status(u_min=2.0, u_max=2.0) == 0
    band = dict(u_min=-1.0, u_max=1.0)
    for kw in (dict(n_layers=0), dict(n_layers=17), dict(n_layers=-1), dict(n_layers=2), dict(n_layers=2, u_min=0.0),
               dict(n_layers=2, u_max=0.0), dict(n_layers=3, u_min=1.0, u_max=1.0),
               dict(n_layers=16, u_min=0.0, u_max=1e-44)):       # 16 / 1e-44 is no float32
        assert status(**kw) == BAD_SIZE, kw
    assert status(n_layers=16, **band) == 0 and status(n_layers=1, **band) == 0
    if d2pc.device_count() == 0:
        assert lib.d2pc_sectors_create(ctypes.byref(good), ctypes.byref(h)) == NO_DEVICE and not h
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.Sectors()
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_config_init(device_id=1 << 20)       # (geometry does not look at the device, create does)
    assert lib.d2pc_sectors_geometry(ctypes.byref(bad), ctypes.byref(g)) == 0
    assert lib.d2pc_sectors_create(ctypes.byref(bad), ctypes.byref(h)) == NO_DEVICE
    bad.device_id = -1
    assert lib.d2pc_sectors_create(ctypes.byref(bad), ctypes.byref(h)) == NO_DEVICE


def test_desc_refusals_without_a_device():
    """d2pc_sectors_desc_check is d2pc_sectors_process_device's own check (csrc/d2pc_sectors_plan.hpp); the pointers
    are numbers here, nothing is dereferenced."""
    cfg = d2pc.sectors_config_init()     # 72 cells: outputs of 288 / 288 / 288 / 144 bytes
    P, C, R, N, K, D = 0x10000000, 0x20000000, 0x30000000, 0x30001000, 0x30002000, 0x30003000
    n = 1000
    good = dict(points=P, counts=C, cloud_points=n, range=R, count=N, nearest=K, distance_cm=D)

    def status(cfg=cfg, **kw):
        return d2pc.sectors_desc_check(cfg, d2pc.sectors_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    assert status() == 0 and status(point_step=32) == 0 and status(counts=None) == 0
    assert lib.d2pc_sectors_desc_check(ctypes.byref(cfg), None) == INVALID_ARG
    assert lib.d2pc_sectors_desc_check(None, ctypes.byref(d2pc.sectors_desc_init(**good))) == INVALID_ARG
    assert status(cfg=d2pc.sectors_config_init(n_sectors=7)) == INVALID_ARG
    assert status(struct_size=76) == INVALID_ARG and status(points=None) == INVALID_ARG
    for step in (0, 8, 12, 24, 48, 64, -16):
        assert status(point_step=step) == INVALID_ARG, step
    for k in (0, -1, 65536):
        assert status(n_clouds=k, points_frame_stride_points=n) == INVALID_ARG, k
    assert status(points=1 << 44, n_clouds=65535, points_frame_stride_points=n) == 0
    assert status(range=None, count=None, nearest=None, distance_cm=None) == INVALID_ARG
    for only in ("range", "count", "nearest", "distance_cm"):
        assert status(**{k: (good[k] if k == only else None) for k in ("range", "count", "nearest", "distance_cm")}) == 0, only
    # alignment
    assert status(points=P + 8) == INVALID_ARG and status(points=P + 16) == 0
    assert status(counts=C + 2) == INVALID_ARG and status(range=R + 2) == INVALID_ARG and status(count=N + 1) == INVALID_ARG
    assert status(nearest=K + 2) == INVALID_ARG and status(distance_cm=D + 1) == INVALID_ARG and status(distance_cm=D + 2) == 0
    # sizes
    big = 1 << 44
    assert status(cloud_points=0) == BAD_SIZE and status(cloud_points=1 << 32) == BAD_SIZE and status(points=big, cloud_points=1 << 40) == BAD_SIZE
    assert status(points=big, cloud_points=(1 << 32) - 1) == 0                    # its last position is 0xFFFFFFFE
    assert status(n_clouds=3, points_frame_stride_points=n - 1) == BAD_SIZE and status(n_clouds=3, points_frame_stride_points=n) == 0
    assert status(n_clouds=1, points_frame_stride_points=0) == 0                  # one cloud: not looked at
    # the largest position (n_clouds - 1) * stride + cloud_points - 1 stays below 0xFFFFFFFF
    assert status(points=big, n_clouds=2, cloud_points=1 << 31, points_frame_stride_points=(1 << 31) - 1) == BAD_SIZE  # stride < cp
    assert status(points=big, n_clouds=2, cloud_points=1 << 30, points_frame_stride_points=(3 << 30) - 1) == 0   # last: 2^32 - 2
    assert status(points=big, n_clouds=2, cloud_points=1 << 30, points_frame_stride_points=3 << 30) == BAD_SIZE  # last: 2^32 - 1
    assert status(points=big, n_clouds=65535, cloud_points=1, points_frame_stride_points=65539) == BAD_SIZE
    assert status(points=big, n_clouds=65535, cloud_points=1, points_frame_stride_points=65538) == 0   # last: 2^32 - 4
    assert status(points=big, n_clouds=2, cloud_points=5, points_frame_stride_points=1 << 63) == BAD_SIZE
    # overlaps: an output over the records (first, last byte), over counts, over another output
    assert status(range=P) == INVALID_ARG and status(count=P + 16 * n - 4) == INVALID_ARG and status(count=P + 16 * n) == 0
    assert status(point_step=32, count=P + 32 * n - 4) == INVALID_ARG
    assert status(n_clouds=3, points_frame_stride_points=n + 7, nearest=P + 16 * (2 * (n + 7) + n) - 4) == INVALID_ARG
    assert status(n_clouds=3, points_frame_stride_points=n + 7, nearest=P + 16 * (2 * (n + 7) + n)) == 0
    assert status(points=R - 16 * n) == 0 and status(points=R - 16 * n + 16) == INVALID_ARG
    assert status(distance_cm=C) == INVALID_ARG and status(n_clouds=2, points_frame_stride_points=n, distance_cm=C + 6) == INVALID_ARG
    assert status(distance_cm=C + 4) == 0                                        # one cloud: counts is 4 bytes
    assert status(count=R) == INVALID_ARG and status(count=R + 284) == INVALID_ARG and status(count=R + 288) == 0
    assert status(distance_cm=K + 286) == INVALID_ARG and status(nearest=D + 140) == INVALID_ARG and status(nearest=D + 144) == 0
    # the outputs' extent follows the session's cells
    wide = d2pc.sectors_config_init(n_sectors=360, n_layers=16, u_min=0.0, u_max=4.0)
    two = dict(nearest=None, distance_cm=None)
    assert status(cfg=wide, count=R + 4 * 5760 - 4, **two) == INVALID_ARG and status(cfg=wide, count=R + 4 * 5760, **two) == 0
