"""The steer of the obstacle sectors (d2pc_sectors_steer_*) without a GPU: the header, the binding and the exports agree
on the new symbols; the struct sizes; the refusals of create and of d2pc_sectors_steer_desc_check through the library and
again through a stand-alone program under sanitizers; the reach tables and the goal cell against numpy in float64;
tests/sectors_steer_ref.py's direct 2-D window against a separable restatement.  tests/README_sectors_steer.md has the map."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_elev_ref
import sectors_steer_ref as sref
from disparity_to_point_cloud_amd import sectors

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG, BAD_SIZE, CAPACITY, NO_DEVICE = 1, 3, 4, 5
F32 = np.float32
HALF_PI = 1.5707964
STEER_SYMBOLS = ["d2pc_sectors_steer_config_init", "d2pc_sectors_steer_create", "d2pc_sectors_steer_desc_check",
                 "d2pc_sectors_steer_desc_init", "d2pc_sectors_steer_destroy", "d2pc_sectors_steer_device",
                 "d2pc_sectors_steer_goal_cell", "d2pc_sectors_steer_last_error", "d2pc_sectors_steer_reach"]
# grid, steer configuration, the smallest distance of a quotient 100 rho / sin(theta) from an integer a numpy prototype found
CONFIGS = {
    "72x1": (dict(), dict(radius=0.5, max_reach_sectors=8, max_reach_layers=0), 1.1e-2),
    "12x4": (dict(n_sectors=12, n_layers=4, u_min=-2.0, u_max=2.0), dict(radius=0.75, max_reach_sectors=3, max_reach_layers=2), 6.6e-2),
    "8x3": (dict(n_sectors=8, n_layers=3, u_min=-1.5, u_max=1.5), dict(radius=0.75, max_reach_sectors=3, max_reach_layers=2), None),
    "60x30e": (dict(n_sectors=60, n_layers=30, layer_kind=1, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60),
               dict(radius=0.5, max_reach_sectors=8, max_reach_layers=4), 4.7e-3),
    "90x64e": (dict(n_sectors=90, n_layers=64, layer_kind=1, u_min=-1.2, u_max=1.2), dict(radius=1.0, max_reach_sectors=16, max_reach_layers=8), 6.2e-4),
}


def configs(name):
    grid, steer, _ = CONFIGS[name]
    return d2pc.sectors_config_init(**grid), d2pc.sectors_steer_config_init(**steer)


# ------------------------------------------------------------------------------------------------ header, binding, exports
def test_header_binding_and_exports_hold_the_steer_symbols():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "d2pc_sectors.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\b(d2pc_[a-z0-9_]+)\s*\(", src)))
    assert sorted(n for n in declared if "_steer_" in n) == STEER_SYMBOLS
    assert sorted(n for n in sectors.SECTORS_SYMBOLS if "_steer_" in n) == STEER_SYMBOLS
    assert not [n for n in STEER_SYMBOLS if "_memory_" in n]
    lib = d2pc.load_sectors_library()
    out = subprocess.run(["nm", "-D", "--defined-only", d2pc.sectors_library_path()], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    for name in STEER_SYMBOLS:
        assert hasattr(lib, name) and name in exported, name
    assert d2pc.SectorsSteer is sectors.SectorsSteer


def test_struct_sizes_defaults_and_null_sessions(tmp_path):
    """The new structs are pinned, the old ones are what they were, and the C compiler agrees with the binding."""
    assert ctypes.sizeof(d2pc.SectorsConfig) == 80 and ctypes.sizeof(d2pc.SectorsDesc) == 80 and ctypes.sizeof(d2pc.SectorsGeometry) == 72
    old = dict(d2pc_sectors_memory_config=(d2pc.SectorsMemoryConfig, 16), d2pc_sectors_memory_step=(d2pc.SectorsMemoryStep, 64),
               d2pc_sectors_fov=(d2pc.SectorsFov, 40), d2pc_sectors_memory_desc=(d2pc.SectorsMemoryDesc, 104))
    new = dict(d2pc_sectors_steer_config=(d2pc.SectorsSteerConfig, 48), d2pc_sectors_steer_step=(d2pc.SectorsSteerStep, 32),
               d2pc_sectors_steer_candidate=(d2pc.SectorsSteerCandidate, 8), d2pc_sectors_steer_desc=(d2pc.SectorsSteerDesc, 64))
    sizes = dict(old, **new)
    for name, (cls, size) in sizes.items():
        assert ctypes.sizeof(cls) == size, name
    src = tmp_path / "sizes.c"
    src.write_text('#include "d2pc_sectors.h"\n' + "".join(
        "typedef char size_of_%s[sizeof(%s) == %d ? 1 : -1];\n" % (n, n, s) for n, (_, s) in sizes.items()) +
        "typedef char size_of_config[sizeof(d2pc_sectors_config) == 80 && sizeof(d2pc_sectors_desc) == 80 && "
        "sizeof(d2pc_sectors_geometry_t) == 72 ? 1 : -1];\n"
        "typedef char caps[D2PC_SECTORS_STEER_MAX_REACH_SECTORS == 32 && D2PC_SECTORS_STEER_MAX_REACH_LAYERS == 16 && "
        "D2PC_SECTORS_STEER_MAX_CANDIDATES == 32 && D2PC_SECTORS_STEER_MAX_WEIGHT == 4095 && D2PC_SECTORS_STEER_OFF == 0xFFFFFFFFu ? 1 : -1];\n")
    p = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"), "-c",
                        str(src), "-o", str(tmp_path / "sizes.o")], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr
    assert (sectors.STEER_MAX_REACH_SECTORS, sectors.STEER_MAX_REACH_LAYERS, sectors.STEER_MAX_CANDIDATES, sectors.STEER_MAX_WEIGHT,
            sectors.STEER_OFF) == (32, 16, 32, 4095, 0xFFFFFFFF)
    s = d2pc.sectors_steer_config_init()
    assert (s.struct_size, s.radius, s.max_reach_sectors, s.max_reach_layers, s.free_cm, s.min_clearance_cm, s.horizon_cm, s.w_goal,
            s.w_prev, s.w_near, list(s.reserved)) == (48, 0.5, 8, 0, 65535, 100, 1000, 16, 4, 1, [0, 0])
    d = d2pc.sectors_steer_desc_init()
    assert (d.struct_size, d.n_candidates) == (64, 1)
    assert all(getattr(d, k) is None for k in ("distance_cm", "allowed", "step", "clearance_cm", "cost", "candidates", "summary"))
    lib = d2pc.load_sectors_library()
    lib.d2pc_sectors_steer_config_init(None)   # tolerated
    lib.d2pc_sectors_steer_desc_init(None)
    assert lib.d2pc_sectors_steer_last_error(None) == b"null session"
    assert lib.d2pc_sectors_steer_destroy(None) == INVALID_ARG and lib.d2pc_sectors_steer_device(None, ctypes.byref(d), None) == INVALID_ARG
    w = d2pc.sectors_steer_step(3, 1, 0xFFFFFFFF, 7)
    assert w.dtype == np.uint32 and w.tolist() == [3, 1, 0xFFFFFFFF, 7, 0, 0, 0, 0] and np.array_equal(w, sref.step_words(3, 1, 0xFFFFFFFF, 7))
    assert d2pc.sectors_steer_step().tolist() == [0xFFFFFFFF, 0, 0xFFFFFFFF, 0, 0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------------ refusals
def test_create_refusals_and_no_device():
    lib = d2pc.load_sectors_library()
    h, g = ctypes.c_void_p(), d2pc.SectorsGeometry()
    no_gpu = d2pc.device_count() == 0
    ok = NO_DEVICE if no_gpu else 0

    def status(grid=None, struct_size=48, **kw):
        cfg = d2pc.sectors_config_init(**(grid or {}))
        s = d2pc.sectors_steer_config_init(**kw)
        s.struct_size = struct_size
        st = lib.d2pc_sectors_steer_create(ctypes.byref(cfg), ctypes.byref(s), ctypes.byref(h))
        if h:
            lib.d2pc_sectors_steer_destroy(h)
        refused = lib.d2pc_sectors_geometry(ctypes.byref(cfg), ctypes.byref(g))
        if refused:
            assert st == refused, "create refuses the grid as d2pc_sectors_create does"
        desc = d2pc.sectors_steer_desc_init(distance_cm=0x1000, step=0x2000, summary=0x3000)
        if st not in (0, NO_DEVICE):
            assert st == d2pc.sectors_steer_desc_check(cfg, s, desc), "desc_check refuses a configuration as create does"
            assert lib.d2pc_sectors_steer_reach(ctypes.byref(cfg), ctypes.byref(s), (ctypes.c_uint16 * 4096)(), 4096,
                                                (ctypes.c_uint16 * 32)(), 32) == -st
        return st

    good, s = d2pc.sectors_config_init(), d2pc.sectors_steer_config_init()
    assert lib.d2pc_sectors_steer_create(ctypes.byref(good), ctypes.byref(s), None) == INVALID_ARG
    assert lib.d2pc_sectors_steer_create(None, ctypes.byref(s), ctypes.byref(h)) == INVALID_ARG
    assert lib.d2pc_sectors_steer_create(ctypes.byref(good), None, ctypes.byref(h)) == INVALID_ARG and not h
    assert status() == ok and status(max_reach_sectors=0) == ok and status(max_reach_sectors=32) == ok
    assert status(w_goal=4095, w_prev=4095, w_near=4095, free_cm=65535, min_clearance_cm=65535, horizon_cm=65535) == ok
    assert status(w_goal=0, w_prev=0, w_near=0, free_cm=0, min_clearance_cm=0, horizon_cm=0) == ok
    assert status(struct_size=44) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    for kw in (dict(radius=0.0), dict(radius=-0.5), dict(radius=np.nan), dict(radius=np.inf), dict(radius=-np.inf), dict(w_goal=4096),
               dict(w_prev=4096), dict(w_near=4096), dict(free_cm=65536), dict(min_clearance_cm=65536), dict(horizon_cm=65536),
               dict(radius=0.0, max_reach_sectors=33)):                     # INVALID_ARG comes before BAD_SIZE
        assert status(**kw) == INVALID_ARG, kw
    for kw in (dict(max_reach_sectors=33), dict(max_reach_sectors=-1), dict(max_reach_layers=17), dict(max_reach_layers=-1),
               dict(max_reach_layers=1), dict(grid=dict(n_sectors=8), max_reach_sectors=5),
               dict(grid=dict(n_sectors=12, n_layers=4, u_min=-2.0, u_max=2.0), max_reach_sectors=3, max_reach_layers=4)):
        assert status(**kw) == BAD_SIZE, kw
    assert status(grid=dict(n_sectors=8), max_reach_sectors=4) == ok
    assert status(grid=dict(n_sectors=12, n_layers=4, u_min=-2.0, u_max=2.0), max_reach_sectors=6, max_reach_layers=3) == ok
    assert status(grid=dict(n_sectors=90, n_layers=64, layer_kind=1, u_min=-1.2, u_max=1.2), max_reach_sectors=32, max_reach_layers=16) == ok
    # the grid's refusals come first, with the grid's statuses
    assert status(grid=dict(n_sectors=71), max_reach_sectors=99) == INVALID_ARG
    assert status(grid=dict(n_layers=17), radius=0.0) == BAD_SIZE and status(grid=dict(n_layers=2), radius=np.nan) == BAD_SIZE
    assert status(grid=dict(layer_kind=1, u_min=-2.0, u_max=1.0), w_goal=5000) == BAD_SIZE
    if no_gpu:
        with pytest.raises(d2pc.D2pcError) as e:
            d2pc.SectorsSteer(good)
        assert e.value.status == NO_DEVICE
    bad = d2pc.sectors_config_init(device_id=1 << 20)
    assert lib.d2pc_sectors_steer_create(ctypes.byref(bad), ctypes.byref(s), ctypes.byref(h)) == NO_DEVICE and not h


# name -> (base address, bytes per cell, fixed bytes, alignment); the candidates' extent is 8 x n_candidates
BUFFERS = dict(distance_cm=(0x40000000, 2, 0, 2), allowed=(0x40100000, 1, 0, 1), step=(0x40200000, 0, 32, 4),
               clearance_cm=(0x50000000, 2, 0, 2), cost=(0x50100000, 4, 0, 4), candidates=(0x50200000, 0, 40, 8), summary=(0x50300000, 0, 16, 4))
OUTPUTS = ("clearance_cm", "cost", "candidates", "summary")


@pytest.mark.parametrize("grid", [dict(), dict(n_sectors=360, n_layers=16, u_min=0.0, u_max=4.0)], ids=["72", "5760"])
def test_desc_refusals_without_a_device(grid):
    """d2pc_sectors_steer_desc_check is d2pc_sectors_steer_device's own check (csrc/d2pc_sectors_steer_plan.hpp); the
    pointers are numbers here, nothing is dereferenced."""
    cfg, scfg = d2pc.sectors_config_init(**grid), d2pc.sectors_steer_config_init()
    n = cfg.n_sectors * cfg.n_layers
    good = dict({k: v[0] for k, v in BUFFERS.items()}, n_candidates=5)
    size = {k: per * n + fixed for k, (_, per, fixed, _) in BUFFERS.items()}

    def status(cfg=cfg, scfg=scfg, **kw):
        return d2pc.sectors_steer_desc_check(cfg, scfg, d2pc.sectors_steer_desc_init(**dict(good, **kw)))

    lib = d2pc.load_sectors_library()
    desc = d2pc.sectors_steer_desc_init(**good)
    assert status() == 0 and status(allowed=None) == 0
    assert lib.d2pc_sectors_steer_desc_check(ctypes.byref(cfg), ctypes.byref(scfg), None) == INVALID_ARG
    assert lib.d2pc_sectors_steer_desc_check(None, ctypes.byref(scfg), ctypes.byref(desc)) == INVALID_ARG
    assert lib.d2pc_sectors_steer_desc_check(ctypes.byref(cfg), None, ctypes.byref(desc)) == INVALID_ARG
    # the grid's refusals first with the grid's statuses, then the steer configuration's, then the descriptor's
    assert status(cfg=d2pc.sectors_config_init(n_sectors=7), distance_cm=None) == INVALID_ARG
    assert status(cfg=d2pc.sectors_config_init(n_layers=17), scfg=d2pc.sectors_steer_config_init(radius=0.0), distance_cm=None) == BAD_SIZE
    assert status(scfg=d2pc.sectors_steer_config_init(max_reach_sectors=33), distance_cm=None) == BAD_SIZE
    assert status(scfg=d2pc.sectors_steer_config_init(w_near=4096)) == INVALID_ARG
    # each alone
    assert status(struct_size=56) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    assert status(distance_cm=None) == INVALID_ARG and status(step=None) == INVALID_ARG
    assert status(**{k: None for k in OUTPUTS}) == INVALID_ARG
    for only in OUTPUTS:
        assert status(**{k: (good[k] if k == only else None) for k in OUTPUTS}) == 0, only
    for k in (0, -1, 33, 1 << 20):
        assert status(n_candidates=k) == INVALID_ARG, k
        assert status(n_candidates=k, candidates=None) == 0, "n_candidates is not looked at without candidates"
    assert status(n_candidates=1) == 0 and status(n_candidates=32) == 0
    # alignment to the type; candidates to 8 bytes
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
            assert end % align == 0 and (base - size[o]) % align == 0
            assert status(**{o: base - size[o] + align}) == INVALID_ARG, (o, "over the first byte of", b)
            assert status(**{o: base - size[o]}) == 0, (o, "ends where", b, "begins")
            assert status(**{o: end - align}) == INVALID_ARG, (o, "over the last byte of", b)
            assert status(**{o: end}) == 0, (o, "begins where", b, "ends")
    assert status(allowed=None, summary=BUFFERS["allowed"][0] + size["allowed"] - 4) == 0, "a buffer that is not given overlaps nothing"
    # the candidates' extent is n_candidates records
    ca = BUFFERS["candidates"][0]
    assert status(n_candidates=1, summary=ca + 8) == 0 and status(n_candidates=2, summary=ca + 8) == INVALID_ARG
    assert status(n_candidates=32, summary=ca + 248) == INVALID_ARG and status(n_candidates=32, summary=ca + 256) == 0


def test_steer_plan_header_under_address_and_undefined_sanitizers(tmp_path):
    """tests/cpp/sectors_steer_plan_main.cpp, a stand-alone program over csrc/d2pc_sectors_steer_plan.hpp (host code, nothing
    loaded into Python): both refusal matrices, the reach tables filled into exactly their capacity and goal_cell, with
    -fsanitize=address,undefined."""
    exe = tmp_path / "sectors_steer_plan"
    p = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                        "-fno-omit-frame-pointer", "-I", os.path.join(ROOT, "disparity_to_point_cloud_amd", "csrc"),
                        os.path.join(ROOT, "tests", "cpp", "sectors_steer_plan_main.cpp"), "-o", str(exe)], capture_output=True, text=True, timeout=180)
    assert p.returncode == 0, p.stderr
    env = dict(os.environ, ASAN_OPTIONS="abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]


# ------------------------------------------------------------------------------------------------------ the reach tables
@pytest.mark.parametrize("name", list(CONFIGS))
def test_reach_tables_against_numpy(name):
    """Direct numpy evaluation in float64, equality demanded.  Two libms may differ in the last bit of a sine, so the test
    first asserts a CONDITION (not a tolerance): every quotient 100 rho / sin(theta) is exactly an integer or at least 1e-6
    from one, a distance no last-bit difference can cross (the quotients are below 1e5: a relative 1e-15 of them is 1e-10)."""
    cfg, scfg = configs(name)
    want_s, want_l, q = sref.reach_tables(cfg, scfg)
    off = np.abs(q - np.round(q))
    away = off[off != 0]
    print("%s: %d quotients, %d exactly integers, the others at least %.2g from one" % (name, q.size, (off == 0).sum(), away.min()))
    assert q.size and np.all((off == 0) | (off >= 1e-6)), "a quotient lies next to an integer: choose another configuration"
    assert q.max() < 1e5
    noted = CONFIGS[name][2]
    if noted is not None:
        assert 0.5 * noted <= away.min() <= 2.0 * noted, "the prototype's figure (two digits) is not this configuration's"
    got_s, got_l = d2pc.sectors_steer_reach(cfg, scfg)
    assert got_s.dtype == got_l.dtype == np.uint16
    assert got_s.shape == (cfg.n_layers, scfg.max_reach_sectors + 1) and got_l.shape == (scfg.max_reach_layers + 1,)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_l, want_l)
    # a cell always sees itself; monotone non-increasing in k; never below 100 rho
    assert np.all(got_s[:, 0] == 65535) and got_l[0] == 65535
    assert np.all(np.diff(got_s.astype(np.int64), axis=1) <= 0) and np.all(np.diff(got_l.astype(np.int64)) <= 0)
    assert np.all(got_s[:, 1:] <= 65534) and np.all(got_s >= int(100 * scfg.radius)) and np.all(got_l[1:] <= 65534)
    if cfg.layer_kind == d2pc.LAYERS_HEIGHT:
        assert np.all(got_s == got_s[0]), "height layers: every row is the same"
        if scfg.max_reach_layers:
            assert got_l.tolist() == [65535, 65534, 0], "half a slab of 1.0 is below the radius of 0.75, one and a half is not"
    else:
        mid = cfg.n_layers // 2
        assert np.all(got_s[0, 1:] >= got_s[mid, 1:]) and np.all(got_s[-1, 1:] >= got_s[mid, 1:]), "an obstacle near the pole spans more sectors"
    if name == "8x3":
        assert got_s[0].tolist()[3] == 75, "2.5 x 45 degrees is beyond pi / 2: floor(100 rho), exact for a dyadic radius"


def test_reach_clamp_near_the_pole_and_capacities():
    cfg = d2pc.sectors_config_init(**CONFIGS["60x30e"][0])
    scfg = d2pc.sectors_steer_config_init(radius=2.0, max_reach_sectors=8, max_reach_layers=4)
    want_s, want_l, q = sref.reach_tables(cfg, scfg)
    off = np.abs(q - np.round(q))
    assert np.all((off == 0) | (off >= 1e-6))
    got_s, got_l = d2pc.sectors_steer_reach(cfg, scfg)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_l, want_l)
    assert got_s[0, 1] == got_s[-1, 1] == 65534 and q.max() > 65535 and got_s[15, 1] < 65534 and np.all(got_s[:, 1:] <= 65534)
    lib = d2pc.load_sectors_library()
    u16 = ctypes.POINTER(ctypes.c_uint16)
    rs, rl = np.full(30 * 9 + 4, 0xABCD, dtype=np.uint16), np.full(5 + 4, 0xABCD, dtype=np.uint16)
    call = lambda a, na, b, nb: lib.d2pc_sectors_steer_reach(ctypes.byref(cfg), ctypes.byref(scfg), a, na, b, nb)  # noqa: E731
    assert call(rs.ctypes.data_as(u16), 30 * 9 - 1, rl.ctypes.data_as(u16), 5) == -CAPACITY
    assert call(rs.ctypes.data_as(u16), 30 * 9, rl.ctypes.data_as(u16), 4) == -CAPACITY
    assert call(None, 30 * 9, rl.ctypes.data_as(u16), 5) == -INVALID_ARG and call(rs.ctypes.data_as(u16), 30 * 9, None, 5) == -INVALID_ARG
    assert np.all(rs == 0xABCD) and np.all(rl == 0xABCD), "a refused call wrote"
    assert call(rs.ctypes.data_as(u16), 30 * 9, rl.ctypes.data_as(u16), 5) == 30 * 9
    assert np.array_equal(rs[:270].reshape(30, 9), want_s) and np.array_equal(rl[:5], want_l) and np.all(rs[270:] == 0xABCD) and np.all(rl[5:] == 0xABCD)


# ------------------------------------------------------------------------------------------------------ the goal cell
@pytest.mark.parametrize("name", list(CONFIGS))
def test_goal_cell_against_numpy(name):
    """Directions at the cell centres and 1e-6 rad inside every edge, in float64; a yaw several turns away."""
    cfg, _ = configs(name)
    n, layers = cfg.n_sectors, cfg.n_layers
    alpha = 2 * np.pi / n
    elevation = cfg.layer_kind == d2pc.LAYERS_ELEVATION
    if elevation:
        e = sectors_elev_ref.boundary_elevations(cfg.u_min, cfg.u_max, layers)
        pitches = [(i, p) for i in range(layers) for p in ((e[i] + e[i + 1]) / 2, e[i] + 1e-6, e[i + 1] - 1e-6)]
    else:
        pitches = [(i, p) for i in range(layers) for p in (float(i), i + 0.5, i + 1 - 1e-6)]
    some = pitches if n * layers <= 100 else pitches[::7] + pitches[-3:]
    for k in range(n):
        for yaw in (cfg.azimuth0 + (k + 0.5) * alpha, cfg.azimuth0 + k * alpha + 1e-6, cfg.azimuth0 + (k + 1) * alpha - 1e-6):
            want = int(np.floor(np.mod(yaw - cfg.azimuth0, 2 * np.pi) / alpha))
            assert want == k
            for i, p in (some if k % 9 == 0 else some[:2]):
                assert d2pc.sectors_steer_goal_cell(cfg, yaw, p) == (k, i), (yaw, p)
    i, p = pitches[len(pitches) // 2]
    for turns in (-3, 5, 1000):
        yaw = cfg.azimuth0 + 2.5 * alpha + turns * 2 * np.pi
        want = int(np.floor(np.mod(yaw - cfg.azimuth0, 2 * np.pi) / alpha))
        assert want == 2 and d2pc.sectors_steer_goal_cell(cfg, yaw, p) == (2, i)
    lo, hi = (float(F32(cfg.u_min)), float(F32(cfg.u_max))) if elevation else (0.0, float(layers))
    for bad in (lo - 1e-6, hi, hi + 1e-6, np.nan, np.inf):
        with pytest.raises(d2pc.D2pcError) as err:
            d2pc.sectors_steer_goal_cell(cfg, 0.1, bad)
        assert err.value.status == INVALID_ARG
    for bad in (np.nan, np.inf, -np.inf):
        with pytest.raises(d2pc.D2pcError):
            d2pc.sectors_steer_goal_cell(cfg, bad, p)
    lib = d2pc.load_sectors_library()
    s = ctypes.c_uint32(9)
    assert lib.d2pc_sectors_steer_goal_cell(ctypes.byref(cfg), 0.1, p, None, ctypes.byref(s)) == INVALID_ARG
    assert lib.d2pc_sectors_steer_goal_cell(None, 0.1, p, ctypes.byref(s), ctypes.byref(s)) == INVALID_ARG and s.value == 9
    cfg.n_sectors = 7
    assert lib.d2pc_sectors_steer_goal_cell(ctypes.byref(cfg), 0.1, p, ctypes.byref(s), ctypes.byref(s)) == INVALID_ARG


# ----------------------------------------------------------------------------------------- the reference against itself
def separable_clearance(ref, distance_cm):
    """The form the kernel takes, written independently of SectorsSteerRef.clearance: an azimuth pass per layer against the
    layer's own reach_s row, then a layer pass over the first pass's minima against reach_l."""
    d = ref.mapped(distance_cm)
    first = d.copy()
    for k in range(1, ref.wa + 1):
        for v in (np.roll(d, -k, axis=1), np.roll(d, k, axis=1)):
            first = np.where((v <= ref.reach_s[:, k][:, None]) & (v < first), v, first)
    out = first.copy()
    for k in range(1, ref.we + 1):
        up, down = first[k:], first[:-k]                       # the rows l + k of the rows 0 .. L - 1 - k, the rows l - k of k .. L - 1
        out[:-k] = np.where((up <= ref.reach_l[k]) & (up < out[:-k]), up, out[:-k])
        out[k:] = np.where((down <= ref.reach_l[k]) & (down < out[k:]), down, out[k:])
    return out.reshape(-1)


def seeded_grid(ref, rng, occupancy):
    """A grid with `occupancy` of its cells holding an obstacle: half of the values lie on, one above and one below a reach
    entry (every entry of both tables takes part), the others anywhere in 0 .. 65535."""
    entries = np.unique(np.concatenate([ref.reach_s.reshape(-1), ref.reach_l]))
    pool = np.clip(np.concatenate([entries - 1, entries, entries + 1]), 0, 65535)
    n = ref.n_cells
    v = np.where(rng.random(n) < 0.5, pool[rng.integers(0, len(pool), n)], rng.integers(0, 65536, n))
    return np.where(rng.random(n) < occupancy, v, 65535).astype(np.uint16)


@pytest.mark.parametrize("name", list(CONFIGS))
def test_reference_direct_window_equals_the_separable_form(name):
    """200 seeded grids per configuration, occupancy 0 %, 8 %, 50 % and 100 %."""
    cfg, scfg = configs(name)
    ref = sref.SectorsSteerRef(cfg, scfg, *d2pc.sectors_steer_reach(cfg, scfg))
    rng = np.random.default_rng(cfg.n_sectors * 100 + cfg.n_layers)
    widened = 0
    for i in range(200):
        occupancy = (0.0, 0.08, 0.5, 1.0)[i % 4]
        d = seeded_grid(ref, rng, occupancy)
        direct, sep = ref.clearance_window(d), separable_clearance(ref, d)
        assert np.array_equal(direct, sep), "%s grid %d (occupancy %g): cell %d" % (name, i, occupancy, np.flatnonzero(direct != sep)[0])
        if occupancy <= 0.08 or ref.n_cells <= 100:     # the window from the obstacles' side, which clearance() takes where they are few
            assert np.array_equal(ref.clearance_scatter(d), direct), "%s grid %d: the two sides of the window" % (name, i)
        assert np.all(direct <= ref.mapped(d).reshape(-1))
        if occupancy == 0.0:
            assert np.all(direct == 65535)
        widened += int((direct < ref.mapped(d).reshape(-1)).sum())
    assert widened > 200, "the window never reached a neighbour"
