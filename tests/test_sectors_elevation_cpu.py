"""The elevation layers of the obstacle sectors (layer_kind = 1) without a GPU: the ABI's sizes and defaults, every
refusal of the mode, the elevation table against numpy, the geometry, tests/sectors_elev_ref.py against float64 atan2
binning, a grid written out by hand, and the host code under the sanitizers.  tests/README_sectors_elevation.md has the
map."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_elev_ref
import sectors_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, CAPACITY, NO_DEVICE = 1, 3, 4, 5
F32 = np.float32
HALF_PI = float(F32(np.pi / 2))          # 1.5707964f, the float nearest pi / 2: a band's outermost bound
ELEV = dict(layer_kind=d2pc.LAYERS_ELEVATION)
# (u_min, u_max, n_layers, n_sectors): the bands the definition was checked on, each on a grid of its own
GRIDS = [(-HALF_PI, HALF_PI, 30, 60), (-0.5, 0.7, 7, 72), (-1.5707964, 1.5707964, 64, 90), (0.0, 0.3, 1, 72)]


def elev_config(u_min, u_max, n_layers, n_sectors=72, **kw):
    return d2pc.sectors_config_init(**dict(dict(ELEV, u_min=u_min, u_max=u_max, n_layers=n_layers, n_sectors=n_sectors), **kw))


def elev_ref(cfg):
    return sectors_elev_ref.SectorsElevRef(cfg, d2pc.sectors_table(cfg), d2pc.sectors_geometry(cfg), d2pc.sectors_elevation_table(cfg))


# ------------------------------------------------------------------------------------------------ sizes and defaults
def test_struct_sizes_stand_and_the_default_is_height_mode():
    assert ctypes.sizeof(d2pc.SectorsConfig) == 80 and ctypes.sizeof(d2pc.SectorsDesc) == 80 and ctypes.sizeof(d2pc.SectorsGeometry) == 72
    assert d2pc.SectorsConfig.layer_kind.offset == 60 and d2pc.SectorsGeometry.elevation_entries.offset == 28
    assert (d2pc.LAYERS_HEIGHT, d2pc.LAYERS_ELEVATION) == (0, 1)
    c = d2pc.sectors_config_init()
    c.layer_kind = 77
    d2pc.load_sectors_library().d2pc_sectors_config_init(ctypes.byref(c))
    assert c.layer_kind == d2pc.LAYERS_HEIGHT and not any(c.reserved) and len(c.reserved) == 3
    g = d2pc.sectors_geometry(c)
    assert g.elevation_entries == 0 and g.lds_bytes == 72 * 12 + 36 * 8
    lib = d2pc.load_sectors_library()
    fp = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(200, dtype=F32)
    # a configuration of height layers has no elevation table
    assert lib.d2pc_sectors_elevation_table(ctypes.byref(c), buf.ctypes.data_as(fp), buf[100:].ctypes.data_as(fp), 100) == -INVALID_ARG
    with pytest.raises(d2pc.D2pcError):
        d2pc.sectors_elevation_table(c)
    assert not buf.any()


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_of_the_elevation_mode():
    lib = d2pc.load_sectors_library()
    g, h = d2pc.SectorsGeometry(), ctypes.c_void_p()

    def status(**kw):
        cfg = d2pc.sectors_config_init(**kw)
        st = lib.d2pc_sectors_geometry(ctypes.byref(cfg), ctypes.byref(g))
        assert lib.d2pc_sectors_create(ctypes.byref(cfg), ctypes.byref(h)) == (st or (NO_DEVICE if d2pc.device_count() == 0 else 0))
        if h:
            lib.d2pc_sectors_destroy(h)
        return st

    band = dict(ELEV, u_min=-0.5, u_max=0.7)
    assert status(**band) == 0                                          # one layer, and it needs its band
    for kind in (2, -1, 1 << 30):
        assert status(layer_kind=kind) == INVALID_ARG and status(layer_kind=kind, n_layers=0) == INVALID_ARG, kind
    # a layer kind that is none is told before any size; the refusals of arguments keep their rank in elevation mode
    assert status(**dict(band, n_sectors=7)) == INVALID_ARG and status(**dict(band, n_layers=0, min_count=0)) == INVALID_ARG
    for n in (0, -1, 65, 1000):
        assert status(**dict(band, n_layers=n)) == BAD_SIZE, n
    for n in (1, 16, 17, 64):
        assert status(**dict(band, n_layers=n)) == 0, n
    # n_sectors * n_layers <= 5,760
    assert status(**dict(band, n_sectors=90, n_layers=64)) == 0 and status(**dict(band, n_sectors=92, n_layers=64)) == BAD_SIZE
    assert status(**dict(band, n_sectors=360, n_layers=16)) == 0 and status(**dict(band, n_sectors=360, n_layers=17)) == BAD_SIZE
    assert status(**dict(band, n_sectors=192, n_layers=30)) == 0 and status(**dict(band, n_sectors=194, n_layers=30)) == BAD_SIZE
    # the band: within +-1.5707964f, infinities included, and not empty
    above, inf = float(np.nextafter(F32(HALF_PI), F32(2))), float("inf")
    assert status(**dict(ELEV, u_min=-HALF_PI, u_max=HALF_PI)) == 0
    for kw in (dict(u_min=-above, u_max=0.5), dict(u_min=-0.5, u_max=above), dict(u_min=-inf, u_max=0.5), dict(u_min=-0.5, u_max=inf),
               dict(), dict(u_min=-inf, u_max=-inf), dict(u_min=2.0, u_max=3.0), dict(u_min=-3.0, u_max=-2.0),
               dict(u_min=0.25, u_max=0.25), dict(u_min=0.0, u_max=-0.0), dict(u_min=HALF_PI, u_max=HALF_PI)):
        assert status(**dict(ELEV, n_layers=1, **kw)) == BAD_SIZE, kw
        assert status(**dict(ELEV, n_layers=5, **kw)) == BAD_SIZE, kw
    tiny = float(np.nextafter(F32(0.25), F32(1)))
    assert status(**dict(ELEV, n_layers=64, u_min=0.25, u_max=tiny)) == 0     # (no inv_h in this mode: any band that is not empty)
    # NaN and u_min > u_max stay refusals of the argument, as in height mode
    nan = float("nan")
    for kw in (dict(u_min=nan, u_max=0.5), dict(u_min=-0.5, u_max=nan), dict(u_min=0.5, u_max=-0.5), dict(u_min=3.0, u_max=2.0)):
        assert status(**dict(ELEV, **kw)) == INVALID_ARG, kw
    # no status of a height-mode configuration moved: the same arguments with layer_kind = 0
    assert status(n_layers=17) == BAD_SIZE and status(n_layers=16, u_min=-1.0, u_max=1.0) == 0 and status(u_min=2.0, u_max=2.0) == 0
    assert status(n_layers=2) == BAD_SIZE and status(u_min=-inf, u_max=inf) == 0 and status(n_sectors=360, n_layers=16, u_min=0.0, u_max=4.0) == 0
    # the table's own refusals
    fp = ctypes.POINTER(ctypes.c_float)
    buf = np.zeros(200, dtype=F32)
    c, s = buf.ctypes.data_as(fp), buf[100:].ctypes.data_as(fp)
    cfg = elev_config(-0.5, 0.7, 7)
    assert lib.d2pc_sectors_elevation_table(ctypes.byref(cfg), c, s, 7) == -CAPACITY
    assert lib.d2pc_sectors_elevation_table(ctypes.byref(cfg), None, s, 100) == -INVALID_ARG
    assert lib.d2pc_sectors_elevation_table(ctypes.byref(cfg), c, None, 100) == -INVALID_ARG
    assert lib.d2pc_sectors_elevation_table(None, c, s, 100) == -INVALID_ARG
    cfg.n_layers = 65
    assert lib.d2pc_sectors_elevation_table(ctypes.byref(cfg), c, s, 100) == -BAD_SIZE
    assert not buf.any(), "a refused call wrote the table"
    cfg.n_layers = 7
    assert lib.d2pc_sectors_elevation_table(ctypes.byref(cfg), c, s, 8) == 8 and buf[:8].all() and not buf[8:100].any()


# -------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize("n_layers", [1, 7, 30, 64])
@pytest.mark.parametrize("band", [(-HALF_PI, HALF_PI), (-0.5, 0.7), (0.0, 0.3)], ids=["pi/2", "-0.5..0.7", "0..0.3"])
def test_elevation_table_against_numpy_bit_for_bit(band, n_layers):
    cfg = elev_config(band[0], band[1], n_layers)
    ce, se = d2pc.sectors_elevation_table(cfg)
    assert ce.dtype == se.dtype == F32 and len(ce) == len(se) == n_layers + 1 == d2pc.sectors_geometry(cfg).elevation_entries
    lo, hi = np.float64(F32(band[0])), np.float64(F32(band[1]))
    e = lo + (np.arange(n_layers + 1, dtype=np.float64) * (hi - lo)) / np.float64(n_layers)     # in double ...
    assert e[0] == lo and abs(e[-1] - hi) <= 2.3e-16
    assert ce.tobytes() == np.cos(e).astype(F32).tobytes() and se.tobytes() == np.sin(e).astype(F32).tobytes()   # ... then float
    assert np.array_equal(e, sectors_elev_ref.boundary_elevations(band[0], band[1], n_layers))
    if band[0] == 0.0:
        assert ce[0].tobytes() == F32(1.0).tobytes() and se[0].tobytes() == F32(0.0).tobytes()
    if band[0] == -HALF_PI:
        # the float nearest pi / 2 lies beyond pi / 2: the outermost cosines are negative, the sines are -1 and +1
        assert ce[0] == ce[-1] == F32(np.cos(np.float64(F32(HALF_PI)))) and ce[0] < 0 and (se[0], se[-1]) == (-1.0, 1.0)
        if n_layers % 2 == 0:
            assert (ce[n_layers // 2], se[n_layers // 2]) == (1.0, 0.0), "the middle boundary is at elevation exactly 0"


# --------------------------------------------------------------------------------------------------------- geometry
def test_geometry_of_both_kinds():
    g = d2pc.sectors_geometry(elev_config(-HALF_PI, HALF_PI, 30, 60, r_min=0.2, r_max=15.0))
    assert (g.n_cells, g.table_entries, g.elevation_entries, g.blocks_per_cu) == (1800, 30, 31, 4)
    assert g.inv_h == 0.0 and g.rmin2 == F32(0.2) * F32(0.2) and g.rmax2 == 225.0 and g.share_points == 1024
    assert g.lds_bytes == 1800 * 12 + 30 * 8 + 31 * 8 and g.block_bytes == 1800 * 12
    assert g.device_bytes == 4 * 256 * 1800 * 12 + 30 * 8 + 31 * 8
    g = d2pc.sectors_geometry(elev_config(-1.5707964, 1.5707964, 64, 90))
    assert (g.n_cells, g.table_entries, g.elevation_entries, g.blocks_per_cu) == (5760, 45, 65, 2)
    assert g.lds_bytes == 69120 + 360 + 520 and g.block_bytes == 69120 and g.device_bytes == 2 * 256 * 69120 + 360 + 520
    assert g.lds_bytes > 64 * 1024 and 2 * g.lds_bytes <= 160 * 1024
    # a height-mode grid: the formula it always had, to the byte
    kw = dict(n_sectors=72, n_layers=16, u_min=-1.5, u_max=2.5, r_min=0.3, r_max=25.0)
    g = d2pc.sectors_geometry(d2pc.sectors_config_init(**kw))
    assert (g.n_cells, g.table_entries, g.elevation_entries, g.blocks_per_cu) == (1152, 36, 0, 4) and g.inv_h == F32(4.0)
    assert g.lds_bytes == 1152 * 12 + 36 * 8 and g.block_bytes == 1152 * 12 and g.device_bytes == 4 * 256 * 1152 * 12 + 36 * 8
    e = d2pc.sectors_geometry(d2pc.sectors_config_init(**dict(kw, u_min=-0.5, u_max=0.5, **ELEV)))
    assert e.lds_bytes - g.lds_bytes == e.device_bytes - g.device_bytes == 8 * 17 and e.inv_h == 0.0 and e.elevation_entries == 17
    assert bytes(g)[56:] == bytes(16) and bytes(e)[56:] == bytes(16)              # reserved stays zero


# ------------------------------------------------------------------------------------ the reference against atan2
@pytest.mark.parametrize("u_min,u_max,n_layers,n_sectors", GRIDS, ids=["pi/2x30", "-0.5..0.7x7", "1.5707964x64", "0..0.3x1"])
def test_reference_agrees_with_float64_atan2(u_min, u_max, n_layers, n_sectors):
    """200,000 seeded points; those within 1e-4 rad of an elevation or an azimuth boundary are left out (float32
    coordinates and the tables' rounding move a direction by about 1e-7 rad), at most 2 % of them; no mismatch in gate,
    layer or sector among the rest."""
    az = -np.pi / n_sectors
    cfg = elev_config(u_min, u_max, n_layers, n_sectors, azimuth0=az, r_min=0.0, r_max=float("inf"), axes=(1, 2, 3))
    m = 200_000
    xyz = (np.random.default_rng(n_layers).standard_normal((m, 3)) * 6).astype(F32)
    xyz[:1000] *= F32(1e-3)
    xyz[1000:2000, :2] *= F32(1e-4)              # next to the vertical axis
    f, l, u = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    part, cell, d2 = elev_ref(cfg).cells(xyz)
    inside, layer, apart = sectors_elev_ref.atan2_layer(f, l, u, u_min, u_max, n_layers)
    width = 2 * np.pi / n_sectors
    a = np.mod(np.arctan2(l.astype(np.float64), f.astype(np.float64)) - az, 2 * np.pi) / width
    near = (apart < 1e-4) | (np.abs(a - np.round(a)) * width < 1e-4)
    share = near.mean()
    print("excluded share %.4f, inside the band %.4f" % (share, inside.mean()))
    assert share <= 0.02
    keep = ~near
    assert inside[keep].sum() > 1000 and np.array_equal(part[keep], inside[keep]), "gate"
    both = keep & inside
    assert np.array_equal(cell[both] // n_sectors, layer[both]), "layer"
    assert np.array_equal(cell[both] % n_sectors, sectors_ref.atan2_sector(f, l, n_sectors, az)[both]), "sector"
    assert len(np.unique(layer[both])) == n_layers
    assert d2.dtype == F32 and np.array_equal(d2, f * f + l * l + u * u)


# ----------------------------------------------------------------------------------------------- a grid by hand
def test_reference_grid_on_a_hand_made_cloud():
    """4 sectors (0 ahead, 1 left, 2 behind, 3 right) x 2 layers (below / above the horizon) of a band of +-1 rad.  The key
    is the EUCLIDEAN range: of two points with equal r2 the one with the smaller |u| is nearer, and two points with equal
    d2 but different r2 tie, so that the smaller position wins."""
    cfg = elev_config(-1.0, 1.0, 2, 4, azimuth0=-np.pi / 4, r_min=0.0, axes=(1, 2, 3), no_obstacle_cm=901)
    E = 0xFFFFFFFF
    xyz = np.array([[3, 0, 4],       # position 5: ahead, above; r2 9, d2 25
                    [3, 0, 1],       # 7: the same cell and the same r2, d2 10: the nearest, though its position is larger
                    [0, 5, 0],       # 8: left, elevation 0 = the boundary: above; r2 25, d2 25
                    [0, 3, 4],       # 9: the same cell, r2 9 but d2 25 too: the tie goes to position 8
                    [-2, 0, -1],     # 11: behind, below; d2 5
                    [0, 0, -1],      # 12: straight below: no azimuth
                    [1, 0, 3],       # 13: elevation 1.249 rad: above the band
                    [1, 0, -3],      # 14: below it
                    [np.nan, 1, 1]], dtype=F32)
    pos = np.array([5, 7, 8, 9, 11, 12, 13, 14, 15])
    ref = elev_ref(cfg)
    part, cell, d2 = ref.cells(xyz)
    assert part.tolist() == [True] * 5 + [False] * 4 and cell[:5].tolist() == [4, 4, 5, 5, 2] and d2[:5].tolist() == [25, 10, 25, 25, 5]
    g = ref.grid(xyz, pos)
    assert g["count"].tolist() == [0, 0, 1, 0, 2, 2, 0, 0]
    assert g["nearest"].tolist() == [E, E, 11, E, 7, 8, E, E]
    assert g["range"][[2, 4, 5]].tolist() == [np.sqrt(F32(5)), np.sqrt(F32(10)), 5.0] and np.isinf(g["range"][[0, 1, 3, 6, 7]]).all()
    assert g["distance_cm"].tolist() == [901, 901, 223, 901, 316, 500, 901, 901]
    # the same cloud through height layers of the same count: the key is r2, and the two ties fall the other way
    hcfg = d2pc.sectors_config_init(n_sectors=4, n_layers=2, u_min=-5.0, u_max=5.0, azimuth0=-np.pi / 4, r_min=0.0, axes=(1, 2, 3))
    hg = sectors_ref.SectorsRef(hcfg, d2pc.sectors_table(hcfg), d2pc.sectors_geometry(hcfg)).grid(xyz[:5], pos[:5])
    assert hg["nearest"][[4, 5]].tolist() == [5, 9]
    cfg.min_count = 2
    g = elev_ref(cfg).grid(xyz, pos)
    assert g["distance_cm"].tolist() == [901, 901, 901, 901, 316, 500, 901, 901] and g["nearest"][2] == 11


# --------------------------------------------------------------------------------- the host code under sanitizers
def test_plan_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/sectors_plan_main.cpp, a stand-alone program over csrc/d2pc_sectors_plan.hpp (host code, nothing loaded into
    Python): the refusal matrix, the geometry and both table fills, with -fsanitize=address,undefined."""
    exe = tmp_path / "sectors_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sectors_plan_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]
