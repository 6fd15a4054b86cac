"""The relief session of the obstacle sectors (d2pc_sectors_relief_*) without a GPU: the header, the binding and the exports
agree on the new symbols and the other families' lists are what they were; the struct sizes and offsets; every refusal of
geometry, create and d2pc_sectors_relief_desc_check in its documented order, writing nothing; slot_bytes; the plan header as a
stand-alone program under sanitizers; tests/sectors_relief_ref.py's fit from sums against tests/sectors_slope_ref.py's fit from
points, and its window against ONE slope reference over all the window's points; and the three strips by hand.
tests/README_sectors_relief.md has the map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_relief_cases as cases
import sectors_relief_ref as rref
import sectors_slope_ref as sref
import sectors_terrain_ref as tref
import slope_fit_cases as fit_cases
from disparity_to_point_cloud_amd import sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, NO_DEVICE = 1, 3, 5
F32 = np.float32
RELIEF_SYMBOLS = ["d2pc_sectors_relief_create", "d2pc_sectors_relief_desc_check", "d2pc_sectors_relief_desc_init", "d2pc_sectors_relief_destroy",
                  "d2pc_sectors_relief_geometry", "d2pc_sectors_relief_last_error", "d2pc_sectors_relief_reset_device", "d2pc_sectors_relief_state",
                  "d2pc_sectors_relief_update_device"]
# how many names each family held before the relief: its substring -> count (the base family is what no substring selects)
FAMILIES = {"_memory_": 8, "_steer_": 9, "_ground_": 10, "_terrain_": 10, "_slope_": 10}


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_hold_the_relief_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d2pc_sectors.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))
    assert sorted(n for n in declared if "_relief_" in n) == RELIEF_SYMBOLS
    assert sorted(n for n in sectors.SECTORS_SYMBOLS if "_relief_" in n) == RELIEF_SYMBOLS
    assert sorted(declared) == sorted(sectors.SECTORS_SYMBOLS), "the binding's list is the header's"
    assert not [n for n in RELIEF_SYMBOLS if any(f in n for f in FAMILIES) or not n.startswith("d2pc_sectors_")], "no other family's test selects them"
    for family, count in FAMILIES.items():
        assert len([n for n in declared if family in n]) == count, family
    assert len([n for n in declared if "_relief_" not in n and not any(f in n for f in FAMILIES)]) == 11, "the sectors' own"
    lib = d2pc.load_sectors_library()

    def exported(path):
        out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
        return {ln.split()[-1] for ln in out.splitlines()}

    names = exported(d2pc.sectors_library_path())
    for name in RELIEF_SYMBOLS:
        assert hasattr(lib, name) and name in names, name
    assert sorted(n for n in names if n.startswith("d2pc_")) == sorted(declared), "the library exports the header's names and no other"
    product = os.path.join(os.path.dirname(d2pc.sectors_library_path()), "libd2pc.so")
    assert not [n for n in exported(product) if "relief" in n], "libd2pc.so holds nothing of the relief"
    assert d2pc.SectorsRelief is sectors.SectorsRelief
    for name in ("SectorsReliefDesc", "SectorsReliefGeometry", "sectors_relief_desc_init", "sectors_relief_desc_check", "sectors_relief_geometry"):
        assert getattr(d2pc, name) is getattr(sectors, name), name


def test_struct_sizes_offsets_defaults_and_null_sessions(tmp_path):
    sizes = dict(d2pc_sectors_relief_geometry_t=(d2pc.SectorsReliefGeometry, 80), d2pc_sectors_relief_desc=(d2pc.SectorsReliefDesc, 160))
    for name, (cls, size) in sizes.items():
        assert ctypes.sizeof(cls) == size, name
    src = tmp_path / "sizes.c"
    src.write_text('#include <stddef.h>\n#include "d2pc_sectors.h"\n' + "".join(
        "typedef char size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (n, n, s) for n, (_, s) in sizes.items()) +
        "".join("typedef char at_%s[offsetof(d2pc_sectors_relief_desc, %s) == %d ? 1 : -1];\n" % (f, f, getattr(d2pc.SectorsReliefDesc, f).offset)
                for f, _ in d2pc.SectorsReliefDesc._fields_) +
        "".join("typedef char gat_%s[offsetof(d2pc_sectors_relief_geometry_t, %s) == %d ? 1 : -1];\n" % (f, f, getattr(d2pc.SectorsReliefGeometry, f).offset)
                for f, _ in d2pc.SectorsReliefGeometry._fields_))
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "sizes.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert [f for f, _ in d2pc.SectorsReliefDesc._fields_[2:8]] == ["step", "frame_count", "frame_sum", "frame_sum2", "frame_moments", "allowed"]
    assert tuple(f for f, _ in d2pc.SectorsReliefDesc._fields_[8:]) == rref.OUT, "the slope's twelve outputs in its order, then status"
    d = d2pc.sectors_relief_desc_init()
    assert (d.struct_size, d.n_candidates) == (160, 1) and all(getattr(d, k) is None for k, _ in d._fields_[2:])
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_relief_desc_init(None)   # tolerated
    assert lib.d2pc_sectors_relief_last_error(None) == b"null session"
    p, n = ctypes.c_void_p(0x55), ctypes.c_size_t(7)
    assert lib.d2pc_sectors_relief_state(None, ctypes.byref(p), ctypes.byref(n)) == INVALID_ARG and (p.value, n.value) == (0x55, 7)
    assert lib.d2pc_sectors_relief_destroy(None) == INVALID_ARG and lib.d2pc_sectors_relief_reset_device(None, None) == INVALID_ARG
    assert lib.d2pc_sectors_relief_update_device(None, ctypes.byref(d), None) == INVALID_ARG


# ------------------------------------------------------------------------------------------------------ refusals
def test_geometry_and_create_refusals_in_their_order_and_no_device():
    lib = d2pc.load_sectors_library()
    h, g = ctypes.c_void_p(), d2pc.SectorsReliefGeometry()
    no_gpu = d2pc.device_count() == 0
    ok = NO_DEVICE if no_gpu else 0

    def status(ground=None, slope=None, s_size=32, t_size=32, s_reserved=None, t_reserved=None, null=(), **kw):
        gc = d2pc.sectors_ground_config_init(**(ground or {}))
        sc = d2pc.sectors_slope_config_init(**(slope or {}))
        tc = d2pc.sectors_terrain_config_init(**kw)
        sc.struct_size, tc.struct_size = s_size, t_size
        if s_reserved is not None:
            sc.reserved[s_reserved] = 1
        if t_reserved is not None:
            tc.reserved[t_reserved] = 1
        ptrs = [None if k in null else ctypes.byref(c) for k, c in (("g", gc), ("s", sc), ("t", tc))]
        st = lib.d2pc_sectors_relief_create(*ptrs, ctypes.byref(h))
        if h:
            lib.d2pc_sectors_relief_destroy(h)
        ctypes.memset(ctypes.byref(g), 0xA5, ctypes.sizeof(g))
        refused = lib.d2pc_sectors_relief_geometry(*ptrs, ctypes.byref(g))
        assert (st in (0, NO_DEVICE)) == (refused == 0) and (refused == 0 or st == refused), "create refuses what geometry refuses"
        if refused:
            assert bytes(g) == b"\xa5" * ctypes.sizeof(g) and not h, "a refused call wrote"
            desc = d2pc.sectors_relief_desc_init(step=0x1000, frame_count=0x2000, frame_sum=0x3000, frame_sum2=0x4000, frame_moments=0x5000, status=0x9000)
            assert lib.d2pc_sectors_relief_desc_check(*ptrs, ctypes.byref(desc)) == refused, "desc_check refuses a configuration as create does"
            if "g" not in null and "s" not in null:
                sg = d2pc.SectorsSlopeGeometry()
                slope_refused = lib.d2pc_sectors_slope_geometry(ptrs[0], ptrs[1], ctypes.byref(sg))
                assert slope_refused in (0, refused), "d2pc_sectors_slope_geometry's refusals come first, unchanged"
        return st

    gc, sc, tc = d2pc.sectors_ground_config_init(), d2pc.sectors_slope_config_init(), d2pc.sectors_terrain_config_init()
    assert lib.d2pc_sectors_relief_create(ctypes.byref(gc), ctypes.byref(sc), ctypes.byref(tc), None) == INVALID_ARG
    assert lib.d2pc_sectors_relief_geometry(ctypes.byref(gc), ctypes.byref(sc), ctypes.byref(tc), None) == INVALID_ARG
    assert lib.d2pc_sectors_relief_geometry(None, None, None, None) == INVALID_ARG, "a NULL out before all of them"
    assert status() == ok and status(depth=1) == ok and status(depth=16, ground=dict(n_a=46, n_b=46)) == ok
    assert status(ground=dict(n_a=43, n_b=50)) == ok, "2,150 cells pass"
    assert status(ground=dict(n_a=47, n_b=46)) == BAD_SIZE, "2,162 cells are refused"
    assert status(ground=dict(n_a=64, n_b=32)) == ok and status(ground=dict(n_a=64, n_b=64)) == BAD_SIZE
    for null in ("g", "s", "t", "gs", "st", "gst"):
        assert status(null=null) == INVALID_ARG, null
    # 1. d2pc_sectors_slope_geometry's: the ground's, then the slope's, then the table's size
    assert status(ground=dict(n_a=65), slope=dict(sub=3), depth=0) == BAD_SIZE and status(ground=dict(quantum=0.0), depth=17) == INVALID_ARG
    assert status(ground=dict(window=9), s_size=0, t_size=0) == BAD_SIZE and status(ground=dict(min_count=0), depth=0) == INVALID_ARG
    assert status(s_size=28) == INVALID_ARG and status(slope=dict(sub=5), depth=0) == INVALID_ARG, "the slope's INVALID_ARG before the depth's BAD_SIZE"
    assert status(slope=dict(max_slope=np.nan), depth=17) == INVALID_ARG and status(s_reserved=4, depth=17) == INVALID_ARG
    assert status(ground=dict(n_a=64, n_b=64), slope=dict(sub=3)) == INVALID_ARG, "the slope's before its table's size"
    assert status(ground=dict(n_a=64, n_b=64), t_size=0) == BAD_SIZE and status(ground=dict(n_a=47, n_b=46), t_reserved=0) == BAD_SIZE, \
        "more than 2,155 cells before the terrain configuration"
    # 2. the terrain configuration's: struct_size, depth, reserved words
    assert status(t_size=28) == INVALID_ARG and status(t_size=0) == INVALID_ARG
    for depth in (0, -1, 17, 1 << 20):
        assert status(depth=depth) == BAD_SIZE, depth
    for r in range(6):
        assert status(t_reserved=r) == INVALID_ARG, r
    assert status(depth=17, t_reserved=2) == BAD_SIZE and status(depth=17, t_size=0) == INVALID_ARG
    if no_gpu:
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.SectorsRelief(d2pc.sectors_ground_config_init())
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_ground_config_init(device_id=1 << 20)
    assert lib.d2pc_sectors_relief_create(ctypes.byref(bad), ctypes.byref(sc), ctypes.byref(tc), ctypes.byref(h)) == NO_DEVICE and not h


def test_geometry_sizes_and_slot_bytes():
    sc = d2pc.sectors_slope_config_init(max_slope=0.25)
    for n_a, n_b, depth, slot in ((2, 2, 1, 304), (5, 3, 3, 1152), (4, 4, 2, 1216), (6, 3, 16, 1376), (16, 16, 8, 19456), (33, 31, 2, 77760),
                                  (46, 46, 16, 160816), (64, 32, 4, 155648)):
        gc = d2pc.sectors_ground_config_init(n_a=n_a, n_b=n_b, cell_size=0.25, quantum=1.0 / 512.0)
        g = d2pc.sectors_relief_geometry(gc, sc, d2pc.sectors_terrain_config_init(depth=depth))
        n = n_a * n_b
        assert (g.n_cells, g.inv_c, g.headers_offset, g.tables_offset, list(g.reserved)) == (n, 4.0, 0, 256, [0] * 5)
        assert g.slot_bytes == slot == rref.slot_bytes(n) == (76 * n + 15) // 16 * 16 and g.state_bytes == 256 + depth * slot
        assert g.blocks == (n + 15) // 16
        sg = d2pc.sectors_slope_geometry(gc, sc)
        assert (g.scale, g.max_tilt2) == (sg.scale, sg.max_tilt2) == (0.125, 0.0625)
    assert 76 * 15 == 1140 and rref.slot_bytes(15) == 1152 and rref.slot_bytes(2116) == 160816 and (2116 + 15) // 16 == 133 and 2116 % 16 == 4


# name -> (base address, bytes per cell, fixed bytes, alignment)
BUFFERS = dict(step=(0x40000000, 0, 80, 4), frame_count=(0x40100000, 4, 0, 4), frame_sum=(0x40200000, 8, 0, 8), frame_sum2=(0x40300000, 8, 0, 8),
               frame_moments=(0x40400000, 56, 0, 8), allowed=(0x40500000, 1, 0, 1),
               count=(0x50000000, 4, 0, 4), sum=(0x50100000, 8, 0, 8), sum2=(0x50200000, 8, 0, 8), moments=(0x50300000, 56, 0, 8),
               slope_a=(0x50400000, 4, 0, 4), slope_b=(0x50500000, 4, 0, 4), level_q=(0x50600000, 4, 0, 4), resid_q2=(0x50700000, 4, 0, 4),
               flat=(0x50800000, 1, 0, 1), site=(0x50900000, 1, 0, 1), candidates=(0x50A00000, 0, 40, 8), summary=(0x50B00000, 0, 16, 4),
               status=(0x50C00000, 0, 16, 4))
OUTPUTS = rref.OUT


@pytest.mark.parametrize("grid", [dict(), dict(n_a=46, n_b=46), dict(n_a=5, n_b=3)], ids=["256", "2116", "15"])
def test_desc_refusals_without_a_device(grid):
    """d2pc_sectors_relief_desc_check is d2pc_sectors_relief_update_device's own check (csrc/d2pc_sectors_relief_plan.hpp); the
    pointers are numbers here, nothing is dereferenced.  The overlap with a session's state is the stand-alone program's."""
    cfg, scfg, tcfg = d2pc.sectors_ground_config_init(**grid), d2pc.sectors_slope_config_init(), d2pc.sectors_terrain_config_init(depth=3)
    n = cfg.n_a * cfg.n_b
    good = dict({k: v[0] for k, v in BUFFERS.items()}, n_candidates=5)
    size = {k: per * n + fixed for k, (_, per, fixed, _) in BUFFERS.items()}

    def status(cfg=cfg, scfg=scfg, tcfg=tcfg, **kw):
        return d2pc.sectors_relief_desc_check(cfg, scfg, tcfg, d2pc.sectors_relief_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    desc = d2pc.sectors_relief_desc_init(**good)
    assert status() == 0 and status(allowed=None) == 0
    three = [ctypes.byref(cfg), ctypes.byref(scfg), ctypes.byref(tcfg)]
    assert lib.d2pc_sectors_relief_desc_check(*three, None) == INVALID_ARG
    for k in range(3):
        assert lib.d2pc_sectors_relief_desc_check(*[None if i == k else p for i, p in enumerate(three)], ctypes.byref(desc)) == INVALID_ARG
    # the configurations' refusals come first, in geometry's order
    assert status(cfg=d2pc.sectors_ground_config_init(n_a=65), step=None) == BAD_SIZE
    assert status(scfg=d2pc.sectors_slope_config_init(sub=5), tcfg=d2pc.sectors_terrain_config_init(depth=0)) == INVALID_ARG
    assert status(tcfg=d2pc.sectors_terrain_config_init(depth=0), step=None) == BAD_SIZE
    assert status(cfg=d2pc.sectors_ground_config_init(n_a=47, n_b=46), step=None) == BAD_SIZE
    # each alone
    assert status(struct_size=152) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for k in ("step", "frame_count", "frame_sum", "frame_sum2", "frame_moments"):
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
    assert status(count=BUFFERS["frame_count"][0]) == INVALID_ARG and status(moments=BUFFERS["frame_moments"][0]) == INVALID_ARG, "in place is refused"
    fm = BUFFERS["frame_moments"][0]
    assert status(status=fm + 56 * n - 8) == INVALID_ARG and status(status=fm + 56 * n) == 0, "frame_moments is seven planes long"


def test_relief_plan_header_compiles_with_plain_gxx_and_runs_under_sanitizers(tmp_path):
    """csrc/d2pc_sectors_relief_plan.hpp holds no HIP; tests/cpp/sectors_relief_plan_main.cpp, a stand-alone program over it
    (host code, nothing loaded into Python), runs the refusal matrices in their order, the sizes and the state overlap with
    -fsanitize=address,undefined."""
    csrc = os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc")
    assert "hip" not in re.sub(r"//.*", "", open(os.path.join(csrc, "d2pc_sectors_relief_plan.hpp")).read()).lower()
    exe = tmp_path / "sectors_relief_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-I", csrc, os.path.join(ROOT, "tests", "cpp", "sectors_relief_plan_main.cpp"), "-o", str(exe)],
                       capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------------------------- the reference itself
FIT_OUT = ("slope_a", "slope_b", "level_q", "resid_q2", "flat", "fitted")


def from_sums(ref, cells):
    """tests/sectors_relief_ref.py's fit of the sums that SectorsSlopeRef.cells formed from points."""
    planes = rref.frame_planes(cells["sum"], cells["sum2"], cells["moments"], ref.n_cells)
    return rref.fit_from_sums(cells["count"], planes, ref.min_fit, ref.max_spread_q2, ref.scale, ref.max_tilt2)


def assert_same_fit(ref, cell, k, u, w, what):
    want = ref.cells(cell, k, u, w)
    got = from_sums(ref, want)
    for o in FIT_OUT:
        assert np.asarray(got[o]).tobytes() == np.asarray(want[o]).astype(np.asarray(got[o]).dtype).tobytes(), (what, o)
    return want


@pytest.mark.parametrize("sub", [2, 4, 8, 16])
def test_fit_from_sums_equals_the_fit_from_points_on_random_cells(sub):
    """Cells of 0 .. 40 points on random planes, level, steep, collinear and noisy, heights up to the gate's +-32767: every
    output of the fit from sums (the wrapped S, the pre-steps in Python integers) equals SectorsSlopeRef.cells' (S summed
    directly from the points)."""
    rng = np.random.default_rng(sub)
    ref = fit_cases.ref_of(sub=sub, n_a=16, n_b=16, min_count=int(rng.integers(1, 6)))
    n, seen = 256, dict(fitted=0, flat=0, unfit=0, empty=0)
    for trial in range(6):
        per = np.where(rng.random(n) < 0.9, rng.integers(1, 41, n), 0)
        cell = np.repeat(np.arange(n), per)
        m = len(cell)
        u, w = 2 * rng.integers(0, sub, m) - (sub - 1), 2 * rng.integers(0, sub, m) - (sub - 1)
        kind = rng.integers(0, 6, n)[cell]
        u = np.where(kind == 4, u[np.searchsorted(cell, cell)], u)                     # one column: A = 0
        w = np.where(kind == 5, u, w)                                                  # the diagonal: D = 0
        gu, gw, c = rng.integers(-40, 41, n)[cell], rng.integers(-9, 10, n)[cell], rng.integers(-20000, 20001, n)[cell]
        noise = np.where(kind == 1, rng.integers(-30, 31, m), np.where(kind == 2, rng.integers(-3000, 3001, m), 0))
        k = np.clip(c + np.where(kind == 3, 0, gu) * u + gw * w + noise, -32767, 32767)
        want = assert_same_fit(ref, cell, k, u, w, "trial %d" % trial)
        seen["fitted"] += int(want["fitted"].sum())
        seen["flat"] += int(want["flat"].sum())
        seen["unfit"] += int(((want["count"] > 0) & ~want["fitted"]).sum())
        seen["empty"] += int((want["count"] == 0).sum())
    assert min(seen.values()) > 20, seen


def test_fit_from_sums_equals_the_fit_from_points_on_the_built_cells():
    """tests/slope_fit_cases.py's cells, built at each gate and rounding of the fit: from sums as from points."""
    assert len(fit_cases.CASES) > 40
    for case in fit_cases.CASES:
        cfg = dict(case.cfg)
        ref = fit_cases.ref_of(sub=case.sub, n_a=2, n_b=2, **cfg)
        p = np.asarray(case.points, dtype=np.int64).reshape(-1, 3)
        want = assert_same_fit(ref, np.full(len(p), 3), p[:, 2], p[:, 0], p[:, 1], case.name)
        assert want["count"][3] == len(p)


def relief_ref(depth, sub=8, max_slope=0.26794919, **cfg):
    """A relief reference for cells of 0.5 and a quantum of 2^-9 (inv_c = 2, inv_q = 512, both exact): needs no library."""
    c = dict(n_a=4, n_b=3, axes=(1, 2, 3), window=0, rough_cap=65535)
    c.update(cases.JUDGE)
    c.update(cfg)
    geo = type("Geo", (), dict(inv_c=F32(1.0 / cases.CELL), inv_q=F32(1.0 / cases.QUANTUM)))
    return rref.SectorsReliefRef(type("Cfg", (), c), type("SCfg", (), dict(sub=sub, max_slope=max_slope)), geo, depth)


@pytest.mark.parametrize("n_a,n_b,depth", [(5, 3, 3), (9, 7, 1), (12, 9, 4), (6, 6, 16)])
def test_reference_window_equals_one_slope_reference_over_all_the_windows_points(n_a, n_b, depth):
    """Random scroll sequences over the planted world: every update of the relief reference equals, in every output,
    SectorsSlopeRef.cells over the points of the last `depth` anchored frames of the same h0, each moved to the new corner --
    no ring, no slot, no table.  Frames that are not anchored, changes of h0 and jumps that leave no overlap are among the steps."""
    import collections

    rng = np.random.default_rng(1000 * n_a + 10 * n_b + depth)
    ref = relief_ref(depth, n_a=n_a, n_b=n_b, window=1)
    n = n_a * n_b
    frames = collections.deque(maxlen=depth)
    ia, jb, h0, seq = 3, -4, 1.0, 0
    shifted = dropped = unanchored = fitted_later = 0
    for it in range(70):
        r = rng.random()
        if r < 0.55:
            ia, jb = ia + int(rng.integers(-2, 3)), jb + int(rng.integers(-2, 3))
        elif r < 0.62:
            ia, jb = ia + int(rng.integers(-n_a - 1, n_a + 2)), jb + int(rng.integers(-n_b - 1, n_b + 2))
        elif r < 0.7:
            h0 = float(rng.choice([1.0, 2.0]))
        step = cases.corner_step(ia, jb, h0, goal=(int(rng.integers(0, n_a)), int(rng.integers(0, n_b))))
        if r > 0.93:
            step = cases.corner_step(float(rng.choice([np.nan, np.inf, 6e8])), jb, h0)
        pts = cases.frame_points(rng, n_a, n_b, ia, jb)
        frame = cases.sums_of(n, *pts)
        before = ref.state.copy()
        got = ref.update(step, *frame, n_candidates=4)
        if r > 0.93:
            unanchored += 1
            assert np.array_equal(ref.state, before) and got["status"].tolist() == [seq, 0, 0, 0] and not got["count"].any()
            assert np.all(got["slope_a"] == sref.NOT_FITTED) and np.all(got["level_q"] == -(1 << 31)) and np.all(got["resid_q2"] == 0xFFFFFFFF)
            assert not got["moments"].any() and got["summary"].tolist() == [0, 0, 0, 0] and np.all(got["candidates"] == rref.gref.NO_CANDIDATE)
            continue
        seq += 1
        frames.append((h0, ia, jb, pts))
        cell, k, u, w, took = [], [], [], [], 0
        for fh0, fia, fjb, (fc, fk, fu, fw) in frames:
            if fh0 != h0:
                dropped += 1
                continue
            if abs(fia - ia) >= n_a or abs(fjb - jb) >= n_b:
                continue
            took += 1
            shifted += (fia, fjb) != (ia, jb)
            i, j = fc % n_a + fia - ia, fc // n_a + fjb - jb           # the frame's cells as seen from the new corner
            keep = (i >= 0) & (i < n_a) & (j >= 0) & (j < n_b)
            cell.append((j * n_a + i)[keep]), k.append(fk[keep]), u.append(fu[keep]), w.append(fw[keep])
        want = ref.slope.cells(*[np.concatenate(x) for x in (cell, k, u, w)])
        assert got["status"].tolist() == [seq, took, ia & 0xFFFFFFFF, jb & 0xFFFFFFFF], it
        for o in ("count", "sum", "sum2", "moments") + FIT_OUT:
            assert np.asarray(got[o]).tobytes() == np.asarray(want[o]).astype(np.asarray(got[o]).dtype).tobytes(), (it, o)
        assert np.array_equal(got["site"], rref.gref.brute_sites(n_a, n_b, 1, cases.JUDGE["max_step_q"], got["level_q"], got["flat"]))
        assert got["summary"].tolist() == [int(want["count"].sum()), int(want["flat"].sum()), int(got["site"].sum()), int(want["fitted"].sum())]
        alone = from_sums(ref.slope, dict(count=frame[0], sum=frame[1], sum2=frame[2], moments=frame[3]))
        fitted_later += int((got["fitted"] & ~alone["fitted"] & (frame[0] > 0)).sum())
    assert unanchored >= 1 and (depth == 1 or (shifted > 10 and dropped >= 1 and fitted_later > 0)), "depth 1 is the frame alone"


def test_reference_ring_wrap_and_restart():
    ref = relief_ref(3, n_a=2, n_b=2, min_count=1)
    step = cases.corner_step(0, 0)
    one = cases.sums_of(4, [0], [7], [1], [-3])
    slots = []
    for it in range(7):
        got = ref.update(step, *one)
        slots.append(int(np.argmax(ref.headers()[:3, 3])))
        assert got["status"].tolist() == [it + 1, min(it + 1, 3), 0, 0] and got["count"][0] == min(it + 1, 3)
        assert got["moments"].reshape(7, 4)[:, 0].tolist() == [x * min(it + 1, 3) for x in (1, -3, 1, -3, 9, 7, -21)]
    assert slots == [0, 1, 2, 0, 1, 2, 0], "the smallest seq is replaced, the lowest index on a tie"
    assert ref.headers()[3:].sum() == 0, "headers at and beyond depth stay zero"
    planes, count = ref.table(0)
    assert planes[:, 0].view(np.int64).tolist() == [7, 49, 1, -3, 1, -3, 9, 7, -21] and count.tolist() == [1, 0, 0, 0], "the slope slab's order"
    ref.headers()[1, 3] = 0xFFFFFFFF
    got = ref.update(step, *one)
    assert got["status"].tolist() == [1, 1, 0, 0] and got["count"].tolist() == [1, 0, 0, 0]
    assert ref.headers()[:3, 3].tolist() == [1, 0, 0] and not ref.headers()[1:].any()
    assert tref.slot_bytes(4) == 80 and rref.slot_bytes(4) == 304 and len(ref.state) == 256 + 3 * 304


# ------------------------------------------------------------------------------------------------ the example, by hand
def test_three_strips_are_not_fitted_alone_and_fitted_together():
    """One cell, sub 8, quantum 1/512, cell 0.5 (scale 0.0625), min_count 4, max_spread_q2 200.  Three frames each hold a strip,
    u = -5, 1, 7, w = -7 .. 7 odd, k = 100 + 3 u + 2 w.  Each alone: A = 0, not fitted, resid_q2 = the spread of 2 w = 84, NaN
    slopes.  The window of the three: slope_a = 3 * 0.0625, slope_b = 2 * 0.0625, resid_q2 0, level_q 100, flat -- while the
    ground's spread of the same count / sum / sum2 is 300 > 200.  With k = 100 + 5 u the window is fitted and not flat."""
    assert cases.JUDGE["min_count"] == 4 and cases.JUDGE["max_spread_q2"] == 200
    ref = relief_ref(3, n_a=2, n_b=2)
    assert ref.slope.scale == 0.0625
    step = cases.corner_step(0, 0)
    seen = []
    for u in (-5, 1, 7):
        frame = cases.sums_of(4, *cases.strip(u))
        alone = from_sums(ref.slope, dict(count=frame[0], sum=frame[1], sum2=frame[2], moments=frame[3]))
        assert not alone["fitted"][0] and alone["slope_a"][0] == alone["slope_b"][0] == sref.NOT_FITTED and alone["resid_q2"][0] == 84
        assert alone["level_q"][0] == 100 + 3 * u and alone["flat"][0] == 0
        by_points = ref.slope.cells(*cases.strip(u))
        assert not by_points["fitted"][0] and by_points["resid_q2"][0] == 84, "SectorsSlopeRef.cells agrees"
        seen.append(cases.strip(u))
        got = ref.update(step, *frame)
    assert got["status"].tolist() == [3, 3, 0, 0] and got["count"][0] == 24 and got["fitted"][0]
    assert sref.as_float(got["slope_a"])[0] == F32(0.1875) and sref.as_float(got["slope_b"])[0] == F32(0.125)
    assert got["resid_q2"][0] == 0 and got["level_q"][0] == 100 and got["flat"][0] == 1 and got["site"][0] == 1
    assert got["summary"].tolist() == [24, 1, 1, 1]
    want = ref.slope.cells(*[np.concatenate(x) for x in zip(*seen)])
    for o in ("count", "sum", "sum2", "moments") + FIT_OUT:
        assert np.asarray(got[o]).tobytes() == np.asarray(want[o]).astype(np.asarray(got[o]).dtype).tobytes(), o
    mean, spread, flat = tref.cell_outputs(got["count"], got["sum"].view(np.uint64), got["sum2"], 4, 200)
    assert (mean[0], spread[0], flat[0]) == (103, 300, 0), "the terrain's judgement of the same sums: 9 * 26 + 4 * 21 - 3 * 3 - ... = 300 > 200"
    ref.reset()
    for u in (-5, 1, 7):
        got = ref.update(step, *cases.sums_of(4, *cases.strip(u, slope_u=5, slope_w=0)))
    assert got["fitted"][0] and sref.as_float(got["slope_a"])[0] == F32(0.3125) and got["resid_q2"][0] == 0 and got["flat"][0] == 0, "0.3125 > tan 15 degrees"
