"""The slope session of the obstacle sectors (d2pc_sectors_slope_*) without a GPU: the header, the binding and the exports
agree on the new symbols and libd2pc.so holds none of them; the struct sizes and defaults; every refusal of geometry, create
and d2pc_sectors_slope_desc_check in its documented order, writing nothing; the 2,155-cell seam; blocks_per_cu; the plan header
under plain g++ with sanitizers; and tests/sectors_slope_ref.py against answers by hand.  tests/README_sectors_slope.md has
the map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ground_ref as gref
import sectors_slope_ref as sref
from disparity_to_point_cloud_amd import sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, NO_DEVICE = 1, 3, 5
F32 = np.float32
Q = 1.0 / 512.0
EYE, ZERO = np.eye(3), np.zeros(3)
SLOPE_SYMBOLS = ["d2pc_sectors_slope_blocks", "d2pc_sectors_slope_config_init", "d2pc_sectors_slope_create", "d2pc_sectors_slope_desc_check",
                 "d2pc_sectors_slope_desc_init", "d2pc_sectors_slope_destroy", "d2pc_sectors_slope_geometry", "d2pc_sectors_slope_last_error",
                 "d2pc_sectors_slope_of_degrees", "d2pc_sectors_slope_process_device"]


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_hold_the_slope_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d2pc_sectors.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))
    assert sorted(n for n in declared if "_slope_" in n) == SLOPE_SYMBOLS
    assert sorted(n for n in sectors.SECTORS_SYMBOLS if "_slope_" in n) == SLOPE_SYMBOLS
    assert sorted(declared) == sorted(sectors.SECTORS_SYMBOLS), "the binding's list is the header's"
    lib = d2pc.load_sectors_library()

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines()}

    names = exported(d2pc.sectors_library_path())
    for name in SLOPE_SYMBOLS:
        assert hasattr(lib, name) and name in names, name
    product = os.path.join(os.path.dirname(d2pc.sectors_library_path()), "libd2pc.so")
    assert not [n for n in exported(product) if "_slope_" in n or "_sectors_" in n], "libd2pc.so holds nothing of the sectors"
    assert d2pc.SectorsSlope is sectors.SectorsSlope
    for name in ("SectorsSlopeConfig", "SectorsSlopeDesc", "SectorsSlopeGeometry", "sectors_slope_config_init", "sectors_slope_desc_init",
                 "sectors_slope_desc_check", "sectors_slope_geometry", "sectors_slope_of_degrees"):
        assert getattr(d2pc, name) is getattr(sectors, name), name


def test_struct_sizes_defaults_and_null_sessions(tmp_path):
    sizes = dict(d2pc_sectors_slope_config=(d2pc.SectorsSlopeConfig, 32), d2pc_sectors_slope_geometry_t=(d2pc.SectorsSlopeGeometry, 72),
                 d2pc_sectors_slope_desc=(d2pc.SectorsSlopeDesc, 160), d2pc_sectors_ground_step=(d2pc.SectorsGroundStep, 80))
    for name, (cls, size) in sizes.items():
        assert ctypes.sizeof(cls) == size, name
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "d2pc_sectors.h"\n' + "".join(
        "typedef char size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (n, n, s) for n, (_, s) in sizes.items()) +
        "typedef char caps[D2PC_SECTORS_SLOPE_CELL_BYTES == 76 && D2PC_SECTORS_SLOPE_MAX_CELLS == 2155 && D2PC_SECTORS_SLOPE_MOMENTS == 7 && "
        "D2PC_SECTORS_SLOPE_NOT_FITTED == 0x7FC00000u && 2155 * 76 <= 163840 && 2156 * 76 > 163840 ? 1 : -1];\n" +
        "".join("typedef char at_%s[offsetof(d2pc_sectors_slope_desc, %s) == %d ? 1 : -1];\n" % (f, f, getattr(d2pc.SectorsSlopeDesc, f).offset)
                for f, _ in d2pc.SectorsSlopeDesc._fields_) +
        "".join("typedef char gat_%s[offsetof(d2pc_sectors_slope_geometry_t, %s) == %d ? 1 : -1];\n" % (f, f, getattr(d2pc.SectorsSlopeGeometry, f).offset)
                for f, _ in d2pc.SectorsSlopeGeometry._fields_))
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "sizes.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert (sectors.SLOPE_CELL_BYTES, sectors.SLOPE_MAX_CELLS, sectors.SLOPE_MOMENTS, sectors.SLOPE_NOT_FITTED) == (76, 2155, 7, 0x7FC00000)
    assert sref.NOT_FITTED == sectors.SLOPE_NOT_FITTED and np.isnan(sref.as_float([sref.NOT_FITTED])[0])
    c = d2pc.sectors_slope_config_init()
    assert (c.struct_size, c.sub, list(c.reserved)) == (32, 8, [0] * 5)
    assert F32(c.max_slope) == F32(np.tan(np.deg2rad(15.0))) == F32(0.26794919), "tanf(15 degrees), as a literal"
    d = d2pc.sectors_slope_desc_init()
    assert (d.struct_size, d.point_step, d.n_clouds, d.n_candidates, d.cloud_points, d.points_frame_stride_points) == (160, 16, 1, 1, 0, 0)
    assert all(getattr(d, k) is None for k, _ in d._fields_[4:] if k not in ("cloud_points", "points_frame_stride_points"))
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_slope_config_init(None)   # tolerated
    lib.d2pc_sectors_slope_desc_init(None)
    assert lib.d2pc_sectors_slope_last_error(None) == b"null session" and lib.d2pc_sectors_slope_blocks(None) == 0
    assert lib.d2pc_sectors_slope_destroy(None) == INVALID_ARG and lib.d2pc_sectors_slope_process_device(None, ctypes.byref(d), None) == INVALID_ARG
    # of_degrees: (float)tan in double; 0 for what gives none
    for deg in (0.0, 1.0, 15.0, 30.0, 45.0, 89.0):
        assert F32(d2pc.sectors_slope_of_degrees(deg)) == F32(np.tan(deg * np.pi / 180.0)), deg
    assert d2pc.sectors_slope_of_degrees(15.0) == c.max_slope
    for deg in (np.nan, -1.0, 90.0, 180.0, np.inf, -np.inf):
        assert d2pc.sectors_slope_of_degrees(deg) == 0.0, deg


# ------------------------------------------------------------------------------------------------------ refusals
def test_geometry_and_create_refusals_in_their_order_and_no_device():
    lib = d2pc.load_sectors_library()
    h, g = ctypes.c_void_p(), d2pc.SectorsSlopeGeometry()
    no_gpu = d2pc.device_count() == 0
    ok = NO_DEVICE if no_gpu else 0

    def status(ground=None, struct_size=32, reserved=None, null_scfg=False, **kw):
        gc = d2pc.sectors_ground_config_init(**(ground or {}))
        sc = d2pc.sectors_slope_config_init(**kw)
        sc.struct_size = struct_size
        if reserved is not None:
            sc.reserved[reserved] = 1
        scp = None if null_scfg else ctypes.byref(sc)
        st = lib.d2pc_sectors_slope_create(ctypes.byref(gc), scp, ctypes.byref(h))
        if h:
            lib.d2pc_sectors_slope_destroy(h)
        ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
        refused = lib.d2pc_sectors_slope_geometry(ctypes.byref(gc), scp, ctypes.byref(g))
        assert (st in (0, NO_DEVICE)) == (refused == 0) and (refused == 0 or st == refused), "create refuses what geometry refuses"
        if refused:
            assert bytes(g) == b"\xa5" * ctypes.sizeof(g) and not h, "a refused call wrote"
            desc = d2pc.sectors_slope_desc_init(points=0x1000, cloud_points=4, step=0x2000, summary=0x3000)
            assert lib.d2pc_sectors_slope_desc_check(ctypes.byref(gc), scp, ctypes.byref(desc)) == refused, "desc_check refuses a configuration as create does"
        return st

    good_g, good_s = d2pc.sectors_ground_config_init(), d2pc.sectors_slope_config_init()
    assert lib.d2pc_sectors_slope_create(ctypes.byref(good_g), ctypes.byref(good_s), None) == INVALID_ARG
    assert lib.d2pc_sectors_slope_create(None, ctypes.byref(good_s), ctypes.byref(h)) == INVALID_ARG and not h
    assert lib.d2pc_sectors_slope_geometry(ctypes.byref(good_g), ctypes.byref(good_s), None) == INVALID_ARG
    assert lib.d2pc_sectors_slope_geometry(None, None, None) == INVALID_ARG
    assert status() == ok
    for sub in (2, 4, 8, 16):
        assert status(sub=sub) == ok, sub
    assert status(max_slope=0.0) == ok and status(max_slope=3.0e38) == ok and status(max_slope=-0.0) == ok
    assert status(ground=dict(n_a=46, n_b=46, max_points=4096)) == ok and status(ground=dict(n_a=64, n_b=32, max_points=4096)) == ok
    # the slope configuration's own, each INVALID_ARG
    assert status(null_scfg=True) == INVALID_ARG and status(struct_size=28) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for sub in (0, 1, 3, 5, 6, 7, 9, 12, 15, 17, 32, -8, 1 << 30):
        assert status(sub=sub) == INVALID_ARG, sub
    for ms in (np.nan, np.inf, -np.inf, -1e-30, -0.2679):
        assert status(max_slope=ms) == INVALID_ARG, ms
    for r in range(5):
        assert status(reserved=r) == INVALID_ARG, r
    # the order: the ground's refusals first, with their statuses; then the slope's INVALID_ARG; the table's size last
    assert status(ground=dict(n_a=65), sub=3) == BAD_SIZE, "the ground's BAD_SIZE comes before the slope's INVALID_ARG"
    assert status(ground=dict(quantum=0.0), sub=3) == INVALID_ARG and status(ground=dict(window=9), max_slope=np.nan) == BAD_SIZE
    assert status(ground=dict(n_a=64, n_b=64), sub=3) == INVALID_ARG and status(ground=dict(n_a=64, n_b=64), reserved=4) == INVALID_ARG
    assert status(ground=dict(n_a=64, n_b=64)) == BAD_SIZE
    assert status(ground=dict(n_a=47, n_b=46)) == BAD_SIZE and status(ground=dict(n_a=64, n_b=34)) == BAD_SIZE
    if no_gpu:
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.SectorsSlope(d2pc.sectors_ground_config_init())
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_ground_config_init(device_id=1 << 20)
    assert lib.d2pc_sectors_slope_create(ctypes.byref(bad), ctypes.byref(good_s), ctypes.byref(h)) == NO_DEVICE and not h


def test_the_2155_cell_seam_and_geometry():
    """n_cells * 76 <= 163,840: 2,155 cells (the largest, which no n_a x n_b <= 64 x 64 grid hits: 2,150 = 43 x 50 is the
    nearest below, 2,156 = 44 x 49 the first above) -- the plan header's own arithmetic is pinned by the stand-alone program
    below for 2,155 and 2,156 themselves."""
    sc = d2pc.sectors_slope_config_init()
    passing = [(n_a, n_b) for n_a in range(2, 65) for n_b in range(2, 65) if n_a * n_b * 76 <= 163840]
    for n_a in range(2, 65):
        for n_b in (2, 33, 34, 43, 44, 46, 47, 49, 50, 64):
            gc = d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b)
            g = d2pc.SectorsSlopeGeometry()
            st = d2pc.load_sectors_library().d2pc_sectors_slope_geometry(ctypes.byref(gc), ctypes.byref(sc), ctypes.byref(g))
            assert st == (0 if n_a * n_b <= 2155 else BAD_SIZE), (n_a, n_b)
    assert (43, 50) in passing and (44, 49) not in passing and (46, 46) in passing and (64, 32) in passing and (64, 64) not in passing
    assert max(a * b for a, b in passing) == 2150
    # blocks_per_cu from 160 KiB, 4 at the most; blocks by the ground's arithmetic; the sizes
    for (n_a, n_b), per_cu in (((16, 16), 4), ((45, 45), 1), ((46, 46), 1), ((5, 3), 4), ((32, 32), 2), ((26, 26), 3), ((23, 23), 4), ((24, 24), 3)):
        n = n_a * n_b
        assert per_cu == min(4, 163840 // (76 * n))
        for max_points, blocks in ((0, 256 * per_cu), (1, 1), (4096, 1), (4097, 2), (1 << 30, 256 * per_cu)):
            gc = d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b, max_points=max_points)
            g = d2pc.sectors_slope_geometry(gc, sc)
            gg = d2pc.sectors_ground_geometry(gc)
            assert (g.n_cells, g.sub, g.blocks_per_cu, g.blocks, g.lds_bytes) == (n, 8, per_cu, blocks, 76 * n), (n_a, n_b, max_points)
            assert g.block_bytes == (76 * n + 7) // 8 * 8 and g.device_bytes == blocks * g.block_bytes + 14 * n
            assert g.blocks == min(gg.blocks, 256 * per_cu) or gg.blocks_per_cu != per_cu
            assert list(g.reserved) == [0] * 4
    assert d2pc.sectors_slope_geometry(d2pc.sectors_ground_config_init(n_a=5, n_b=3), sc).block_bytes == 1144, "15 cells: 1,140 rounded up"
    # scale and max_tilt2, formed in double of the float32 fields
    for quantum, cell, sub, ms in ((0.002, 0.5, 8, 0.26794919), (Q, 0.5, 8, 0.1), (0.01, 0.3, 16, 1.0), (1e-3, 2.0, 2, 0.0), (Q, 0.25, 4, 3.0e38)):
        gc, s2 = d2pc.sectors_ground_config_init(quantum=quantum, cell_size=cell), d2pc.sectors_slope_config_init(sub=sub, max_slope=ms)
        g = d2pc.sectors_slope_geometry(gc, s2)
        assert g.scale == sref.scale_of(quantum, cell, sub) == float(F32(quantum)) * (2 * sub) / float(F32(cell)), (quantum, cell, sub)
        assert g.max_tilt2 == sref.max_tilt2_of(ms) == float(F32(ms)) ** 2
    assert d2pc.sectors_slope_geometry(d2pc.sectors_ground_config_init(quantum=Q), sc).scale == 0.0625


# name -> (base address, bytes per cell, fixed bytes, alignment); points: 1,000 records
BUFFERS = dict(points=(0x40000000, 0, 16000, 16), counts=(0x40100000, 0, 4, 4), step=(0x40200000, 0, 80, 4), allowed=(0x40300000, 1, 0, 1),
               count=(0x50000000, 4, 0, 4), sum=(0x50100000, 8, 0, 8), sum2=(0x50200000, 8, 0, 8), moments=(0x50300000, 56, 0, 8),
               slope_a=(0x50400000, 4, 0, 4), slope_b=(0x50500000, 4, 0, 4), level_q=(0x50600000, 4, 0, 4), resid_q2=(0x50700000, 4, 0, 4),
               flat=(0x50800000, 1, 0, 1), site=(0x50900000, 1, 0, 1), candidates=(0x50A00000, 0, 40, 8), summary=(0x50B00000, 0, 16, 4))
OUTPUTS = sref.OUT


@pytest.mark.parametrize("grid", [dict(), dict(n_a=46, n_b=46), dict(n_a=5, n_b=3)], ids=["256", "2116", "15"])
def test_desc_refusals_without_a_device(grid):
    """d2pc_sectors_slope_desc_check is d2pc_sectors_slope_process_device's own check (csrc/d2pc_sectors_slope_plan.hpp); the
    pointers are numbers here, nothing is dereferenced."""
    cfg, scfg = d2pc.sectors_ground_config_init(**grid), d2pc.sectors_slope_config_init()
    n = cfg.n_a * cfg.n_b
    good = dict({k: v[0] for k, v in BUFFERS.items()}, n_candidates=5, cloud_points=1000)
    size = {k: per * n + fixed for k, (_, per, fixed, _) in BUFFERS.items()}

    def status(cfg=cfg, scfg=scfg, **kw):
        return d2pc.sectors_slope_desc_check(cfg, scfg, d2pc.sectors_slope_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    desc = d2pc.sectors_slope_desc_init(**good)
    assert status() == 0 and status(allowed=None, counts=None) == 0 and status(point_step=32) == 0
    assert lib.d2pc_sectors_slope_desc_check(ctypes.byref(cfg), ctypes.byref(scfg), None) == INVALID_ARG
    assert lib.d2pc_sectors_slope_desc_check(None, ctypes.byref(scfg), ctypes.byref(desc)) == INVALID_ARG
    assert lib.d2pc_sectors_slope_desc_check(ctypes.byref(cfg), None, ctypes.byref(desc)) == INVALID_ARG
    # the configurations' refusals come first, the ground's before the slope's
    assert status(cfg=d2pc.sectors_ground_config_init(n_a=65), points=None) == BAD_SIZE
    assert status(cfg=d2pc.sectors_ground_config_init(quantum=0.0), cloud_points=0) == INVALID_ARG
    assert status(scfg=d2pc.sectors_slope_config_init(sub=5), cloud_points=0) == INVALID_ARG
    assert status(cfg=d2pc.sectors_ground_config_init(n_a=64, n_b=64), points=None) == BAD_SIZE
    # each alone
    assert status(struct_size=136) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for kw in (dict(point_step=12), dict(point_step=0), dict(n_clouds=0), dict(n_clouds=65536), dict(points=None), dict(step=None)):
        assert status(**kw) == INVALID_ARG, kw
    assert status(**{k: None for k in OUTPUTS}) == INVALID_ARG
    for only in OUTPUTS:
        assert status(**{k: (good[k] if k == only else None) for k in OUTPUTS}) == 0, only
    for k in (0, -1, 33, 1 << 20):
        assert status(n_candidates=k) == INVALID_ARG, k
        assert status(n_candidates=k, candidates=None) == 0, "n_candidates is not looked at without candidates"
    assert status(n_candidates=1) == 0 and status(n_candidates=32) == 0
    # alignment to the type; sum, sum2, moments and candidates to 8 bytes, points to 16
    for k, (base, _, _, align) in BUFFERS.items():
        for off in range(1, align):
            assert status(**{k: base + off}) == INVALID_ARG, (k, off)
        assert status(**{k: base + align}) == 0, k
    # the cloud sizes, after every INVALID_ARG of the pointers
    assert status(cloud_points=0) == BAD_SIZE and status(cloud_points=1 << 32) == BAD_SIZE
    assert status(cloud_points=(1 << 32) - 1, points=0x7000_0000_0000) == 0, "2^32 - 1 records, placed beyond every other buffer"
    assert status(n_clouds=2, points_frame_stride_points=999) == BAD_SIZE and status(n_clouds=2, points_frame_stride_points=1000) == 0
    assert status(n_clouds=3, points_frame_stride_points=1 << 31) == BAD_SIZE
    assert status(cloud_points=0, step=None) == INVALID_ARG and status(cloud_points=0, moments=BUFFERS["moments"][0] + 4) == INVALID_ARG
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
    mo = BUFFERS["moments"][0]
    assert status(summary=mo + 56 * n - 8) == INVALID_ARG and status(summary=mo + 56 * n) == 0, "moments is seven planes long"


PLAN_MAIN = r"""
#include <cstdio>
#include <cstring>
#include <cmath>
#include <cstdint>
#include "d2pc_sectors.h"
#include "d2pc_sectors_slope_plan.hpp"
using namespace d2pc::sectors;
int main() {
  d2pc_sectors_ground_config g;
  memset(&g, 0, sizeof g);
  g.struct_size = sizeof g, g.n_a = 46, g.n_b = 46, g.cell_size = 0.5f, g.quantum = 0.001953125f;
  g.axes[0] = 1, g.axes[1] = 2, g.axes[2] = 3, g.min_count = 4, g.window = 1;
  d2pc_sectors_slope_config s;
  memset(&s, 0, sizeof s);
  s.struct_size = sizeof s, s.sub = 8, s.max_slope = 0.25f;
  SlopePlan p;
  char msg[256] = "";
  int bad = 0;
  if (make_slope_plan(&g, &s, &p, msg, sizeof msg) != D2PC_OK || p.lds_bytes != 160816 || p.blocks_per_cu != 1 || p.scale != 0.0625 || p.max_tilt2 != 0.0625) bad |= 1;
  g.n_a = 64, g.n_b = 64;
  if (make_slope_plan(&g, &s, &p, msg, sizeof msg) != D2PC_ERR_BAD_SIZE || !strstr(msg, "2155")) bad |= 2;
  s.sub = 3;
  if (make_slope_plan(&g, &s, &p, msg, sizeof msg) != D2PC_ERR_INVALID_ARG || !strstr(msg, "sub")) bad |= 4;
  // the seam itself: the static_assert of the header holds 2,155 and 2,156; restated
  if (size_t(2155) * kSlopeCellBytes > kLdsPerCu || size_t(2156) * kSlopeCellBytes <= kLdsPerCu) bad |= 8;
  // a descriptor: an unaligned moments, then two outputs that overlap, with their messages
  g.n_a = 5, g.n_b = 3, s.sub = 8;
  if (make_slope_plan(&g, &s, &p) != D2PC_OK || p.block_bytes != 1144) bad |= 16;
  d2pc_sectors_slope_desc d;
  memset(&d, 0, sizeof d);
  d.struct_size = sizeof d, d.point_step = 16, d.n_clouds = 1, d.n_candidates = 1, d.cloud_points = 10;
  d.points = (const void *)0x10000, d.step = (const d2pc_sectors_ground_step *)0x20000, d.moments = (int64_t *)0x30004;
  if (check_slope_desc(p, &d, msg, sizeof msg) != D2PC_ERR_INVALID_ARG || !strstr(msg, "moments")) bad |= 32;
  d.moments = (int64_t *)0x30000, d.flat = (uint8_t *)(0x30000 + 7 * 15 * 8 - 1);
  if (check_slope_desc(p, &d, msg, sizeof msg) != D2PC_ERR_INVALID_ARG || !strstr(msg, "overlap")) bad |= 64;
  d.flat = (uint8_t *)(0x30000 + 7 * 15 * 8);
  if (check_slope_desc(p, &d, msg, sizeof msg) != D2PC_OK) bad |= 128;
  if (slope_of_degrees(45.0) != 1.0f || slope_of_degrees(-1.0) != 0.0f || slope_of_degrees(NAN) != 0.0f) bad |= 256;
  printf("bad %d\n", bad);
  return bad ? 1 : 0;
}
"""


def test_the_plan_header_under_plain_gxx_with_sanitizers(tmp_path):
    """csrc/d2pc_sectors_slope_plan.hpp needs no HIP: a stand-alone program of it under -fsanitize=address,undefined."""
    src, exe = tmp_path / "slope_plan_main.cpp", tmp_path / "slope_plan_main"
    src.write_text(PLAN_MAIN)
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc"), str(src), "-o",
                        str(exe)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "bad 0", r.stdout + r.stderr


# ------------------------------------------------------------------------------------------------ the reference, by hand
class Geo:
    inv_c, inv_q = F32(2.0), F32(512.0)


def ref_of(sub=8, max_slope=0.26794919, geo=Geo, **cfg):
    """A reference for cells of 0.5 and a quantum of 2^-9 (inv_c = 2, inv_q = 512, both exact): needs no library."""
    c = dict(n_a=4, n_b=3, cell_size=0.5, quantum=Q, axes=(1, 2, 3), min_count=1, max_spread_q2=625, max_step_q=50, window=0, w_dist=1, w_rough=1,
             rough_cap=65535)
    c.update(cfg)
    return sref.SectorsSlopeRef(type("Cfg", (), c), type("SCfg", (), dict(sub=sub, max_slope=max_slope)), geo)


def cell_points(i, j, us, ws, ks, sub=8, h0=0.0):
    """Records at the centres of the sub-steps (u, w) of cell (i, j) with heights h0 + k quanta."""
    us, ws, ks = np.asarray(us), np.asarray(ws), np.asarray(ks)
    a = (i + ((us + sub - 1) / 2 + 0.5) / sub) * 0.5
    b = (j + ((ws + sub - 1) / 2 + 0.5) / sub) * 0.5
    return np.stack([a, b, h0 + ks * Q], axis=1).astype(F32)


def test_step_9_positions_are_odd_and_exact():
    r = ref_of()
    us = np.arange(-7, 8, 2)
    uu, ww = np.meshgrid(us, us)
    xyz = cell_points(2, 1, uu.ravel(), ww.ravel(), 0 * uu.ravel())
    part, cell, k, u, w = r.bin(xyz, sref.step_words(EYE, ZERO, ZERO))
    assert part.all() and np.all(cell == 1 * 4 + 2) and np.array_equal(u, uu.ravel()) and np.array_equal(w, ww.ravel())
    # the sub-step boundaries belong to the step they begin; the cell's own boundary to the cell it begins
    edge = np.array([[1.0, 0.5, 0.0], [1.0 + 0.0625, 0.5 + 3 * 0.0625, 0.0], [np.nextafter(F32(1.5), F32(0)), np.nextafter(F32(1.0), F32(0)), 0.0]], dtype=F32)
    part, cell, k, u, w = r.bin(edge, sref.step_words(EYE, ZERO, ZERO))
    assert part.all() and cell.tolist() == [6, 6, 6] and u.tolist() == [-7, -5, 7] and w.tolist() == [-7, -1, 7]
    for sub in (2, 4, 16):
        part, cell, k, u, w = ref_of(sub=sub).bin(edge, sref.step_words(EYE, ZERO, ZERO))
        assert u.tolist() == [-(sub - 1), -(sub - 1) + 2 * (sub // 8), sub - 1] and w.tolist() == [-(sub - 1), -(sub - 1) + 2 * (3 * sub // 8), sub - 1]


def test_points_exactly_on_a_plane_give_the_exact_slope():
    """heights h0 + q (c + 3 u - 2 w), cell_size 0.5, quantum 2^-9, P 8: slope_a = 3 * 0.0625 = 0.1875, slope_b = -0.125,
    resid_q2 = 0, level_q = c."""
    r = ref_of(min_count=4)
    assert r.scale == 0.0625
    us = np.arange(-7, 8, 2)
    uu, ww = [x.ravel() for x in np.meshgrid(us, us)]
    for c, h0 in ((100, 0.0), (-3000, 0.0), (0, 12.5), (7, -3.25)):
        xyz = cell_points(1, 2, uu, ww, c + 3 * uu - 2 * ww, h0=h0)
        out = r.process(xyz, sref.step_words(EYE, ZERO, [0, 0, h0]))
        cell = 2 * 4 + 1
        assert out["count"][cell] == 64 and out["fitted"][cell] and out["fitted"].sum() == 1
        assert sref.as_float(out["slope_a"])[cell] == F32(0.1875) and sref.as_float(out["slope_b"])[cell] == F32(-0.125)
        assert out["resid_q2"][cell] == 0 and out["level_q"][cell] == c
        assert out["flat"][cell] == 1, "0.1875^2 + 0.125^2 = 0.0508 <= tan(15 deg)^2 = 0.0718"
        assert out["moments"].reshape(7, 12)[:, cell].tolist() == [0, 0, 64 * 21, 0, 64 * 21, 3 * 64 * 21, -2 * 64 * 21]
        assert out["summary"].tolist() == [64, 1, 1, 1]
        others = np.arange(12) != cell
        assert np.all(out["slope_a"][others] == sref.NOT_FITTED) and np.all(out["level_q"][others] == -(1 << 31)) and np.all(out["resid_q2"][others] == 0xFFFFFFFF)
    # the same plane seen through a subset that is not symmetric: still exact (every quantity is a small integer)
    pick = np.array([0, 5, 9, 14, 27, 33, 62])
    xyz = cell_points(1, 2, uu[pick], ww[pick], 40 + 3 * uu[pick] - 2 * ww[pick])
    out = r.process(xyz, sref.step_words(EYE, ZERO, ZERO))
    assert sref.as_float(out["slope_a"])[9] == F32(0.1875) and sref.as_float(out["slope_b"])[9] == F32(-0.125)
    assert out["resid_q2"][9] == 0 and out["level_q"][9] == 40
    # steeper than max_slope: fitted, smooth, not flat
    xyz = cell_points(1, 2, uu, ww, 5 * uu)
    out = r.process(xyz, sref.step_words(EYE, ZERO, ZERO))
    assert sref.as_float(out["slope_a"])[9] == F32(0.3125) and out["resid_q2"][9] == 0 and out["flat"][9] == 0 and out["summary"].tolist() == [64, 0, 0, 1]


def test_cells_that_are_not_fitted_and_the_level_cell():
    r = ref_of(n_a=4, n_b=3, min_count=1)
    gr = r.ground                                   # the ground reference of the same configuration
    us = np.arange(-7, 8, 2)
    uu, ww = [x.ravel() for x in np.meshgrid(us, us)]
    rng = np.random.default_rng(3)
    clouds = [
        cell_points(0, 0, np.full(8, 3), us, 10 + 2 * us),                      # one u: A = 0
        cell_points(1, 0, [-7, 7], [-7, 7], [5, 9]),                            # 2 points
        cell_points(2, 0, us, us, 20 + us),                                     # on the diagonal: D = 0
        cell_points(3, 0, uu, ww, 50 + rng.integers(-6, 7, 64)),                # level, rough: about 14 quanta^2
        cell_points(0, 1, uu, ww, np.full(64, -77)),                            # level, smooth
        cell_points(1, 1, [-7, 7, -7], [-7, -7, 7], [0, 14, -28]),              # 3 points: the smallest fit, exact
        cell_points(2, 1, [1], [1], [123]),                                     # 1 point
    ]
    xyz = np.concatenate(clouds)
    step = sref.step_words(EYE, ZERO, ZERO)
    out = r.process(xyz, step)
    g = gr.process(xyz, step)
    assert out["count"].tobytes() == g["count"].tobytes() and out["sum"].tobytes() == g["sum"].tobytes() and out["sum2"].tobytes() == g["sum2"].tobytes()
    assert out["fitted"].tolist() == [0, 0, 0, 1, 1, 1, 0, 0, 0, 0, 0, 0]
    for cell in (0, 1, 2, 6):                       # points, not fitted: NaN slopes, the ground's mean_q and spread_q2, never flat
        assert out["slope_a"][cell] == out["slope_b"][cell] == sref.NOT_FITTED
        assert out["level_q"][cell] == g["mean_q"][cell] and out["resid_q2"][cell] == g["spread_q2"][cell] and out["flat"][cell] == 0
    assert g["flat"][0] == 1 and g["flat"][6] == 1, "the ground calls them flat: it cannot know"
    # the level cells: slope 0 (to rounding), the outputs equal the ground's
    assert out["slope_a"][4] in (0, 0x80000000) and out["slope_b"][4] in (0, 0x80000000)
    assert out["level_q"][4] == g["mean_q"][4] == -77 and out["resid_q2"][4] == g["spread_q2"][4] == 0 and out["flat"][4] == 1
    assert abs(int(out["level_q"][3]) - int(g["mean_q"][3])) <= 1 and out["resid_q2"][3] <= g["spread_q2"][3] and out["resid_q2"][3] >= g["spread_q2"][3] - 3
    assert np.all(np.abs(sref.as_float(out["slope_a"])[[3]]) < 0.02)
    # three points: the plane through them, k = -7 + u - 2 w
    assert sref.as_float(out["slope_a"])[5] == F32(0.0625) and sref.as_float(out["slope_b"])[5] == F32(-0.125)
    assert out["resid_q2"][5] == 0 and out["level_q"][5] == -7 and out["flat"][5] == 1
    assert out["summary"].tolist() == [8 + 2 + 8 + 64 + 64 + 3 + 1, 3, 3, 3]
    # min_count above 3 is the fit's too
    out = ref_of(min_count=4).process(xyz, step)
    assert out["fitted"].tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0, 0] and out["level_q"][5] == -5, "floor(-14 / 3)"


def test_a_smooth_slope_and_a_rough_level_cell_come_apart():
    """The point of the feature, on the reference: a 15 degree slope and a level cell with noise of the same spread."""
    n = 64 * 64
    rng = np.random.default_rng(15)
    a, b = rng.uniform(0.0, 0.5, n), rng.uniform(0.0, 0.5, n)
    tilt = np.stack([a, b, 1.0 + (a - 0.25) * np.tan(np.deg2rad(15.0))], axis=1)
    rough = np.stack([a + 0.5, b, 1.0 + rng.normal(0.0, 0.5 * np.tan(np.deg2rad(15.0)) / np.sqrt(12.0), n)], axis=1)
    cfg = dict(n_a=2, n_b=2, quantum=0.002, min_count=4, max_spread_q2=625)
    geo = type("G", (), dict(inv_c=F32(2.0), inv_q=F32(1.0 / float(F32(0.002)))))
    r = ref_of(max_slope=np.tan(np.deg2rad(20.0)), geo=geo, **cfg)
    xyz = np.concatenate([tilt, rough]).astype(F32)
    step = sref.step_words(EYE, ZERO, [0, 0, 1.0])
    out, g = r.process(xyz, step), r.ground.process(xyz, step)
    assert abs(int(g["spread_q2"][0]) - int(g["spread_q2"][1])) < 0.1 * g["spread_q2"][0] and g["flat"][0] == g["flat"][1] == 1, "the ground cannot tell them apart"
    sa, sb = sref.as_float(out["slope_a"]), sref.as_float(out["slope_b"])
    assert abs(sa[0] - np.tan(np.deg2rad(15.0))) < 0.01 and abs(sb[0]) < 0.01 and out["resid_q2"][0] < 0.1 * g["spread_q2"][0], "steep and smooth"
    assert abs(sa[1]) < 0.01 and abs(sb[1]) < 0.01 and out["resid_q2"][1] > 0.9 * g["spread_q2"][1], "level and rough"
    assert out["flat"][0] == 1 and out["flat"][1] == 1
    steep = ref_of(max_slope=np.tan(np.deg2rad(10.0)), geo=geo, **cfg)
    assert steep.process(xyz, step)["flat"].tolist() == [0, 1, 0, 0], "max_slope of 10 degrees refuses the slope and keeps the rubble"
