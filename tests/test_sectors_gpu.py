"""d2pc_sectors_process_device on the GPU.  The clouds are crafted in device memory (no producer is needed to reach a
seam); the expected cells come from tests/sectors_ref.py with the library's own boundary table and inv_h; every
comparison is of bit patterns; every output is sentinel-filled with guard entries behind it.
tests/README_sectors.md has the map of cases."""
import ctypes
import itertools

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
F32 = np.float32
GUARD = 16
OUTPUTS = ("range", "count", "nearest", "distance_cm")
SENTINEL = dict(range=0x7FC3C3C3, count=0x5A5AA5A5, nearest=0x3C3CC3C3, distance_cm=0xA5C3)   # no call here produces them
DTYPE = dict(range=np.uint32, count=np.uint32, nearest=np.uint32, distance_cm=np.uint16)
SIGNED = dict(range=np.int32, count=np.int32, nearest=np.int32, distance_cm=np.int16)     # (torch has no unsigned 16 / 32)
SPECIAL = np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FC0BEEF, 0x7F800000, 0xFF800000], dtype=np.uint32)  # NaNs, +-inf

_sessions = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sessions():
    yield
    for sec, _ in _sessions.values():
        sec.close()
    _sessions.clear()


def session(**kw):
    """(Sectors, SectorsRef) of a configuration, made once per module."""
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))
    if key not in _sessions:
        sec = d2pc.Sectors(**kw)
        _sessions[key] = (sec, sectors_ref.SectorsRef(sec.cfg, d2pc.sectors_table(sec.cfg), sec.geometry))
    return _sessions[key]


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_words(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(DEV)


def fresh_outputs(n_cells, want=OUTPUTS):
    return {k: torch.from_numpy(np.full(n_cells + GUARD, SENTINEL[k], dtype=DTYPE[k]).view(SIGNED[k])).to(DEV) for k in want}


def read_outputs(out, n_cells):
    """-> the outputs as numpy (bit patterns); asserts the guard entries behind each."""
    got = {}
    for k, t in out.items():
        a = t.cpu().numpy().view(DTYPE[k])
        assert np.all(a[n_cells:] == SENTINEL[k]), "%s: an entry past n_cells was written" % k
        got[k] = a[:n_cells].copy()
    return got


def run(sec, points, cloud_points, n_clouds=1, stride=0, counts=None, step=16, want=OUTPUTS, out=None):
    """One call on a device tensor of records -> the outputs asked for, as numpy bit patterns."""
    out = out or fresh_outputs(sec.n_cells, want)
    sec.process(points, cloud_points, point_step=step, n_clouds=n_clouds, counts=counts, frame_stride_points=stride,
                stream_ptr=stream(), **out)
    torch.cuda.synchronize()
    return read_outputs(out, sec.n_cells)


def same(got, want, what=""):
    for k, a in got.items():
        w = want[k].view(DTYPE[k]) if k == "range" else want[k].astype(DTYPE[k])
        bad = np.flatnonzero(a != w)
        assert bad.size == 0, "%s %s: cell %d is 0x%x, not 0x%x (%d cells differ)" % (what, k, bad[0], a[bad[0]], w[bad[0]], bad.size)


def check(sec, ref, words, cloud_points, n_clouds=1, stride=0, counts=None, step=16, want=OUTPUTS, what=""):
    """Upload `words` (records x step / 4 uint32), run, compare with the reference over the records the call visits."""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, step // 4)
    d_counts = dev_words(np.asarray(counts, dtype=np.uint32)) if counts is not None else None
    got = run(sec, dev_words(words), cloud_points, n_clouds, stride, d_counts, step, want)
    xyz, pos = sectors_ref.gather(words, step // 4, n_clouds, cloud_points, stride, counts)
    grid = ref.grid(xyz, pos)
    same(got, grid, what)
    return grid


def records(xyz, step=16, seed=0):
    """xyz float32 (n, 3) -> uint32 records: the pad word and a textured record's second half are arbitrary bits."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=(len(xyz), step // 4), dtype=np.uint64).astype(np.uint32)
    w[:, :3] = np.ascontiguousarray(xyz, dtype=F32).view(np.uint32)
    return w


def random_xyz(n, seed, spread=6.0):
    return (np.random.default_rng(seed).normal(size=(n, 3)) * spread).astype(F32)


def from_flu(axes, f, l, u):
    """The xyz whose picks are f, l, u."""
    xyz = np.zeros((len(f), 3), dtype=F32)
    for a, v in zip(axes, (f, l, u)):
        xyz[:, abs(a) - 1] = -np.asarray(v, dtype=F32) if a < 0 else np.asarray(v, dtype=F32)
    return xyz


BODY = dict(axes=(1, 2, 3), r_min=0.0)       # x forward, y left, z up: f, l, u = x, y, z


# --------------------------------------------------------------------------------------------------- record counts
def test_record_counts_across_the_seams_of_wave_block_and_share():
    """1 .. 257 records (a wave, a block), a share of 1,024 records -1 / +0 / +1, and enough for two shares per block plus
    a ragged third; the default grid.  One cloud in memory, cells() once, every prefix reduced on its own."""
    sec, ref = session()
    share = sec.geometry.share_points
    assert share == 1024 and sec.blocks >= 1
    most = 2 * sec.blocks * share + 3
    xyz = random_xyz(most, seed=1)
    words = records(xyz)
    pts = dev_words(words)
    part, cell, r2 = ref.cells(xyz)
    assert part.sum() > most // 2 and (~part).sum() > 100          # r_min = 0.2 drops some
    pos = np.arange(most, dtype=np.uint32)
    for n in (1, 63, 64, 65, 255, 256, 257, share - 1, share, share + 1, sec.blocks * share - 1, sec.blocks * share + 1, most):
        got = run(sec, pts, n)
        same(got, ref.reduce(part[:n], cell[:n], r2[:n], pos[:n]), "n=%d" % n)
    # the same prefixes through `counts` (read on the device) under a larger cloud_points
    for n in (0, 1, 257, share + 1, most - 1):
        got = run(sec, pts, most, counts=dev_words(np.array([n], dtype=np.uint32)))
        same(got, ref.reduce(part[:n], cell[:n], r2[:n], pos[:n]), "count=%d" % n)


# ------------------------------------------------------------------------------------------------- layouts and counts
@pytest.mark.parametrize("step", [16, 32])
@pytest.mark.parametrize("n_clouds", [1, 3])
def test_record_and_cloud_layouts(step, n_clouds):
    sec, ref = session(n_sectors=72, n_layers=3, u_min=-4.0, u_max=5.0, r_min=1.0, r_max=12.0)
    cp, stride = 2500, 2500 + 37
    words = records(random_xyz(n_clouds * stride, seed=step + n_clouds), step, seed=3)
    grid = check(sec, ref, words, cp, n_clouds, stride, None, step)
    assert (grid["count"] > 0).sum() > 150 and grid["count"].sum() < n_clouds * cp
    if n_clouds == 1:
        assert int(grid["nearest"][grid["count"] > 0].max()) < cp
    else:
        assert int(grid["nearest"][grid["count"] > 0].max()) >= 2 * stride     # a position counts the stride


def test_counts_null_ragged_clamped_failed_and_zero():
    sec, ref = session(n_sectors=72, n_layers=3, u_min=-4.0, u_max=5.0, r_min=1.0, r_max=12.0)
    cp, stride = 1500, 1600
    words = records(random_xyz(3 * stride, seed=11))
    check(sec, ref, words, cp, 3, stride, None)
    check(sec, ref, words, cp, 3, stride, [5, 1500, 777], what="ragged")
    check(sec, ref, words, cp, 3, stride, [1501, 0xFFFFFFFE, 1 << 31], what="clamped")
    check(sec, ref, words, cp, 3, stride, [0xFFFFFFFF, 9, 0xFFFFFFFF], what="failure mark")
    grid = check(sec, ref, words, cp, 3, stride, [0, 0xFFFFFFFF, 0], what="empty")
    assert np.isinf(grid["range"]).all() and not grid["count"].any() and np.all(grid["nearest"] == 0xFFFFFFFF)
    assert np.all(grid["distance_cm"] == 65535)
    sec2, ref2 = session(no_obstacle_cm=1234)
    assert np.all(check(sec2, ref2, words, cp, 3, stride, [0, 0, 0])["distance_cm"] == 1234)


# ---------------------------------------------------------------------------------------------- occupancy patterns
def points_in_cells(ref, cfg, cells, seed, radius=None):
    """A point inside each of the given cells of a BODY-axes grid, in the given order."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells)
    sector, layer = cells % ref.n, cells // ref.n
    width = 2 * np.pi / ref.n
    theta = cfg.azimuth0 + (sector + rng.uniform(0.2, 0.8, size=len(cells))) * width
    r = rng.uniform(1.0, 20.0, size=len(cells)) if radius is None else np.full(len(cells), radius)
    h = (float(cfg.u_max) - float(cfg.u_min)) / ref.layers if ref.layers > 1 else 1.0
    u = (float(cfg.u_min) if ref.layers > 1 else 0.0) + (layer + rng.uniform(0.2, 0.8, size=len(cells))) * h
    return np.stack([r * np.cos(theta), r * np.sin(theta), u], axis=1).astype(F32)


PATTERNS = ["one_cell", "one_point_per_cell", "alternating_lanes", "runs_3", "runs_64", "runs_65", "random"]


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_layers", [1, 3])
def test_occupancy_patterns(pattern, n_layers):
    """72 x 1 cells take the wave's pre-reduction, 72 x 3 the per-lane LDS atomics alone."""
    sec, ref = session(n_sectors=72, n_layers=n_layers, u_min=-1.0, u_max=2.0, azimuth0=0.3, **BODY)
    n_cells, n = ref.n_cells, 4096
    rng = np.random.default_rng(21)
    if pattern == "one_cell":
        cells = np.full(n, 50)
    elif pattern == "one_point_per_cell":
        cells = rng.permutation(n_cells)
    elif pattern == "alternating_lanes":
        cells = np.where(np.arange(n) % 2 == 0, 17, n_cells - 13) + (np.arange(n) // 64 % 3)     # two cells inside every wave
    elif pattern.startswith("runs_"):
        run_len = int(pattern[5:])
        cells = np.repeat(rng.integers(0, n_cells, size=n // run_len + 1), run_len)[:n]
    else:
        cells = rng.integers(0, n_cells, size=n)
    xyz = points_in_cells(ref, sec.cfg, cells, seed=22)
    if pattern == "one_cell":
        xyz[:] = xyz[0]                 # equal r2 everywhere: the nearest is the smallest position ...
        xyz[:7, :2] *= F32(1.5)         # ... and that is not record 0
    part, got_cells, _ = ref.cells(xyz)
    assert part.all() and np.array_equal(got_cells, cells), "the pattern is not the one that was meant"
    grid = check(sec, ref, records(xyz), len(xyz), what=pattern)
    assert np.array_equal(grid["count"], np.bincount(cells, minlength=n_cells))
    if pattern == "one_cell":
        assert grid["count"][50] == n and grid["nearest"][50] == 7
    if pattern == "one_point_per_cell":
        assert np.all(grid["count"] == 1) and np.array_equal(grid["nearest"], np.argsort(cells))


def test_one_point_per_cell_of_the_largest_grid():
    """360 x 16 cells: 70,560 bytes of LDS per block, beyond the 64 KB a launch gets without asking."""
    sec, ref = session(n_sectors=360, n_layers=16, u_min=-2.0, u_max=6.0, azimuth0=-np.pi / 360, **BODY)
    assert sec.geometry.lds_bytes == 70560 and sec.geometry.blocks_per_cu == 2
    cells = np.random.default_rng(23).permutation(ref.n_cells)
    xyz = points_in_cells(ref, sec.cfg, cells, seed=24)
    grid = check(sec, ref, records(xyz), len(xyz))
    assert np.all(grid["count"] == 1) and np.array_equal(grid["nearest"], np.argsort(cells))
    check(sec, ref, records(random_xyz(30000, seed=25, spread=3.0)), 30000, what="random")


# ------------------------------------------------------------------------------------------------------- boundaries
def boundary_points(ref, axes):
    """Points exactly on every boundary direction (the table's own (c_j, s_j) and its opposite, scaled by powers of
    two), the next float on either side in f and in l, and l = +-0 with f of either sign."""
    f, l = [], []
    for scale in (F32(0.125), F32(1.0), F32(32.0)):
        for sign in (F32(1.0), F32(-1.0)):
            c, s = ref.c * scale * sign, ref.s * scale * sign         # (a power of two and a sign: exact)
            for df, dl in itertools.product((-1, 0, 1), repeat=2):
                f.append(c if df == 0 else np.nextafter(c, F32(df) * F32(np.inf)))
                l.append(s if dl == 0 else np.nextafter(s, F32(dl) * F32(np.inf)))
    f.append(np.array([3.0, 3.0, -3.0, -3.0, 1e-15, -1e-15], dtype=F32))
    l.append(np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0], dtype=F32))
    f, l = np.concatenate(f).astype(F32), np.concatenate(l).astype(F32)
    return from_flu(axes, f, l, np.zeros_like(f))


@pytest.mark.parametrize("az", ["0", "-pi/n", "0.3"])
@pytest.mark.parametrize("n", [2, 4, 72, 360])
def test_boundaries(n, az):
    azimuth0 = {"0": 0.0, "-pi/n": -np.pi / n, "0.3": 0.3}[az]
    sec, ref = session(n_sectors=n, azimuth0=azimuth0, **BODY)
    xyz = boundary_points(ref, BODY["axes"])
    _, cell, _ = ref.cells(xyz)
    assert len(np.unique(cell)) == n, "every sector has a point on or next to its boundary"
    check(sec, ref, records(xyz), len(xyz))
    # every point on its own (count 1 in its own cell: a wrong bin cannot hide behind a right count) is the `nearest` test:
    grid = check(sec, ref, records(xyz[::-1]), len(xyz), what="reversed")
    assert grid["count"].sum() == len(xyz)


AXES = [(sf * 1, sl * 2, su * 3) for sf in (1, -1) for sl in (1, -1) for su in (1, -1)] + [(3, -1, -2), (-2, 3, 1)]


@pytest.mark.parametrize("axes", AXES, ids=lambda a: "%+d%+d%+d" % a)
def test_axes(axes):
    sec, ref = session(n_sectors=72, n_layers=3, u_min=-5.0, u_max=7.0, azimuth0=0.3, r_min=0.0, axes=axes)
    xyz = np.concatenate([boundary_points(ref, axes), random_xyz(3000, seed=31)])
    grid = check(sec, ref, records(xyz), len(xyz))
    # what the picks mean: the same cloud expressed in the body frame gives the same grid
    body, bref = session(n_sectors=72, n_layers=3, u_min=-5.0, u_max=7.0, azimuth0=0.3, **BODY)
    f, l, u = ref.flu(xyz)
    want = bref.grid(np.stack([f, l, u], axis=1), np.arange(len(xyz)))
    assert all(np.array_equal(grid[k].view(np.uint32) if k == "range" else grid[k], want[k].view(np.uint32) if k == "range" else want[k])
               for k in OUTPUTS)


# ------------------------------------------------------------------------------------------------------------ gates
def on_circle(r2_bits, seed, tries=4000):
    """(f, l) float32 pairs whose fl(fl(f f) + fl(l l)) has exactly the given bit pattern."""
    rng = np.random.default_rng(seed)
    target = float(np.array([r2_bits], dtype=np.uint32).view(F32)[0])
    f = (np.sqrt(target) * rng.uniform(0.1, 0.95, size=tries)).astype(F32)
    l0 = np.sqrt(np.maximum(target - f.astype(np.float64) ** 2, 0)).astype(F32)
    found = []
    for step in range(-6, 7):
        l = l0.view(np.int32) + step
        l = l.astype(np.int32).view(F32)
        hit = (f * f + l * l).view(np.uint32) == r2_bits
        found.append(np.stack([f[hit], l[hit]], axis=1))
    found = np.concatenate(found)
    assert len(found) >= 3, "no point found on the circle"
    return found[:8]


@pytest.mark.parametrize("n_layers", [1, 3, 16])
def test_gates(n_layers):
    u_min, u_max = F32(-0.7), F32(1.9)
    sec, ref = session(n_sectors=72, n_layers=n_layers, u_min=float(u_min), u_max=float(u_max), azimuth0=0.3, axes=(1, 2, 3),
                       r_min=0.5, r_max=25.0)
    g = sec.geometry
    lo, hi = (int(np.array([v], dtype=F32).view(np.uint32)[0]) for v in (g.rmin2, g.rmax2))
    assert (g.rmin2, g.rmax2) == (0.25, 625.0)
    fl = np.concatenate([on_circle(b, seed=b & 0xFFFF) for b in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1)])
    xyz = [from_flu((1, 2, 3), fl[:, 0], fl[:, 1], np.full(len(fl), 0.5))]
    part = ref.cells(xyz[0])[0]
    assert part.any() and (~part).any()
    # the height gate and every slab edge: u_min, u_max, u_min + k / inv_h, and the floats next to each
    edges = [u_min, u_max] + [F32(u_min + F32(k) / F32(g.inv_h)) for k in range(1, n_layers)] if n_layers > 1 else [u_min, u_max]
    us = np.array([v for e in edges for v in (np.nextafter(e, F32(-np.inf)), e, np.nextafter(e, F32(np.inf)))], dtype=F32)
    if n_layers > 1:
        us = np.concatenate([us, [F32(u_min + F32(k + 0.5) / F32(g.inv_h)) for k in range(n_layers)]]).astype(F32)
    xyz.append(from_flu((1, 2, 3), np.full(len(us), 2.0), np.linspace(-3, 3, len(us)), us))
    # non-finite coordinates: NaN payloads and +-inf in each of x, y, z; the origin; coordinates whose squares vanish
    bad = np.tile(np.array([[2.0, 1.0, 0.5]], dtype=F32), (3 * len(SPECIAL), 1))
    for i, bits in enumerate(np.tile(SPECIAL, 3)):
        bad[i, i // len(SPECIAL)] = np.array([bits], dtype=np.uint32).view(F32)[0]
    xyz.append(bad)
    xyz.append(np.array([[0, 0, 0.5], [-0.0, 0.0, 0.5], [1e-30, -1e-30, 0.5], [1e-45, 0, 0.5], [2.0, 1.0, 0.5]], dtype=F32))
    xyz = np.concatenate(xyz)
    grid = check(sec, ref, records(xyz), len(xyz))
    part, cell, _ = ref.cells(xyz)
    assert not part[-5:-1].any() and part[-1] and not part[-5 - len(bad):-5].any()
    if n_layers > 1:
        assert set(np.unique(cell[part] // 72)) == set(range(n_layers)), "every slab holds a point"
    assert grid["count"].sum() == part.sum()


def test_gates_without_bounds():
    """r_min = 0 and r_max = +inf: r2 that overflows takes part (range +inf, 65534 cm), a subnormal r2 takes part (its
    square root is exact), r2 that underflows to 0 does not; huge |u| passes a gate of -inf .. +inf."""
    sec, ref = session(n_sectors=4, azimuth0=-np.pi / 4, r_max=float("inf"), **BODY)
    xyz = np.array([[1e30, 1.0, 0.0], [-3e38, -1e38, 3e38], [0.0, 2.0 ** -70, -3e38], [0.0, -(2.0 ** -74), 0.0], [2.0 ** -75, 0.0, 0.0],
                    [-1e-45, 1e-45, 0.0], [0.0, 1.5e19, 0.0], [0.0, 1.9e19, 0.0]], dtype=F32)
    grid = check(sec, ref, records(xyz), len(xyz))
    assert grid["count"].tolist() == [1, 3, 1, 1] and grid["nearest"].tolist() == [0, 2, 1, 3]
    assert np.isinf(grid["range"][0]) and grid["range"][1] == F32(2.0 ** -70) and grid["range"][3] == F32(2.0 ** -74)
    assert grid["distance_cm"].tolist() == [65534, 0, 65534, 0]


# ---------------------------------------------------------------------------------------------------------- outputs
@pytest.mark.parametrize("min_count", [1, 3])
def test_outputs_alone_and_together_and_min_count(min_count):
    sec, ref = session(n_sectors=72, azimuth0=-np.pi / 72, min_count=min_count, no_obstacle_cm=3001, **BODY)
    # ranges that end in x.995 m (the truncation), beyond 655.34 m (the clamp), and sectors with 1, 2, 3 and more points
    cells = np.concatenate([np.arange(72), np.arange(0, 72, 2), np.arange(0, 72, 4), np.repeat(np.arange(0, 72, 8), 3)])
    xyz = points_in_cells(ref, sec.cfg, cells, seed=42)
    radii = np.array([2.995, 7.995, 655.33, 655.34, 655.35, 655.345, 700.0, 1e6, 0.004, 0.0051], dtype=F32)
    xyz[:72, :2] *= (radii[np.arange(72) % len(radii)] / np.hypot(xyz[:72, 0], xyz[:72, 1]).astype(F32))[:, None]
    xyz[72:, :2] *= F32(2000.0)         # everything else lies behind the first 72
    words = records(xyz)
    grid = check(sec, ref, words, len(xyz))
    assert set(grid["count"].tolist()) == {1, 2, 3, 6} and (grid["distance_cm"] == 65534).any()
    masked = grid["count"] < min_count
    assert (~masked).any() and masked.any() == (min_count > 1)
    assert np.isinf(grid["range"][masked]).all() and np.all(grid["distance_cm"][masked] == 3001)
    assert np.all(grid["nearest"] != 0xFFFFFFFF) and np.all(grid["count"] >= 1), "count and nearest are not masked"
    pts = dev_words(words)
    for k in OUTPUTS:
        same(run(sec, pts, len(xyz), want=(k,)), grid, "alone")
    same(run(sec, pts, len(xyz), want=("range", "distance_cm")), grid, "two")


def test_truncation_and_clamp_values():
    """The cm forms on exact ranges (l = 0: r2 = f f, and sqrtf(f f) = f)."""
    sec, ref = session(n_sectors=2, azimuth0=-np.pi / 2, **BODY)
    for f, cm in ((2.995, 299), (3.0, 300), (0.0049, 0), (655.33, 65533), (655.34, 65534), (655.35, 65534), (1e9, 65534)):
        grid = check(sec, ref, records(np.array([[f, 0, 0]], dtype=F32)), 1)
        assert grid["range"][0] == F32(f) and grid["distance_cm"].tolist() == [int(min(65534, float(F32(f) * F32(100.0)))), 65535]
        assert abs(int(grid["distance_cm"][0]) - cm) <= 1      # (the decimal in this table, give or take float32's rounding of it)


# ------------------------------------------------------------------------------------------------------ determinism
def test_same_bytes_again_and_after_another_call():
    sec, ref = session(n_sectors=72, n_layers=3, u_min=-4.0, u_max=5.0, r_min=1.0, r_max=12.0)
    n = 3 * sec.blocks * 1024 // 2 + 77
    a, b = dev_words(records(random_xyz(n, seed=51))), dev_words(records(random_xyz(5000, seed=52, spread=2.0)))
    first = run(sec, a, n)
    second = run(sec, a, n)
    other = run(sec, b, 5000)
    third = run(sec, a, n)
    for k in OUTPUTS:
        assert first[k].tobytes() == second[k].tobytes() == third[k].tobytes(), k
    assert other["count"].tobytes() != first["count"].tobytes()


# ------------------------------------------------------------------------------------- behind the producers (end to end)
PT_SENTINEL = 0x7FC5A5A5


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q(), border=3, compact_algo=1) as c:
        yield c


def disparities(f, h, w, seed, holes=0.3):
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 64.0, size=(f, h, w)).astype(F32)
    d[rng.random(size=d.shape) < holes] = 0.0
    return d


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def test_producer_and_sectors_in_one_captured_chain(ctx):
    """d2pc_process_device (COMPACT) -> d2pc_sectors_process_device on the capture stream: one linear chain, no warm-up
    of this session, replayed twice with new input.  A call that allocated would break the capture."""
    h, w, border, f = 37, 70, 3, 3
    roi_n = (h - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    sec, ref = session(n_sectors=36, n_layers=3, u_min=-3.0, u_max=3.0, r_min=0.5, r_max=40.0, min_count=2)
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_COMPACT)
    ctx.set_q(d2pc.make_q(cx=35.0, cy=18.0))
    d = torch.zeros((f, h, w), dtype=torch.float32, device=DEV)
    pts = torch.full((f * stride, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros((f,), dtype=torch.int32, device=DEV)
    out = fresh_outputs(sec.n_cells)

    def both():
        s = stream()
        ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, f, pts.data_ptr(), None, stride,
                           counts.data_ptr(), s)
        sec.process(pts, roi_n, n_clouds=f, counts=counts, frame_stride_points=stride, stream_ptr=s, **out)

    ctx.reserve(w, h, f)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        both()
    torch.cuda.synchronize()
    read_outputs(out, 0)            # capturing ran nothing: every entry still holds its sentinel
    seen = []
    for seed in (61, 62):
        d.copy_(torch.from_numpy(disparities(f, h, w, seed)))
        g.replay()
        torch.cuda.synchronize()
        got = read_outputs(out, sec.n_cells)
        cn = u32(counts)
        assert np.all(cn > 0) and np.all(cn < roi_n)
        xyz, pos = sectors_ref.gather(u32(pts).reshape(-1, 4), 4, f, roi_n, stride, cn)
        grid = ref.grid(xyz, pos)
        same(got, grid, "replay %d" % seed)
        assert grid["count"].sum() > roi_n
        seen.append(got["count"].tobytes())
    assert seen[0] != seen[1], "the replays saw the same input"
    ctx.check_async_error()
    del g
    ctx.release_graph_buffers()
    ctx.set_q(d2pc.make_q())


def pose(yaw_deg, t):
    a = np.deg2rad(yaw_deg)
    m = np.eye(4)
    m[0, 0], m[0, 2], m[2, 0], m[2, 2] = np.cos(a), np.sin(a), -np.sin(a), np.cos(a)     # about the optical frame's y (down)
    m[:3, 3] = t
    return m


def test_rig_to_sectors(ctx):
    """3 posed cameras, COMPACT, one merged cloud; counts = d_offsets + 3 (the total, read on the device)."""
    n, h, w, border = 3, 37, 70, 3
    roi_n = (h - 2 * border) * (w - 2 * border)
    cap = n * roi_n
    q = d2pc.make_q(cx=35.0, cy=18.0)
    qs = [d2pc.rig_compose_q(pose(yaw, t), q) for yaw, t in ((0, (0.1, 0, 0)), (120, (0, 0, -0.1)), (-120, (-0.1, 0.02, 0)))]
    disp = disparities(n, h, w, seed=71)
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_COMPACT)
    d = torch.from_numpy(disp).to(DEV)
    pts = torch.full((cap + GUARD, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    sec, ref = session(r_min=0.5)            # the default grid: 72 sectors, a camera's optical frame
    out = fresh_outputs(sec.n_cells)
    with d2pc.RigSession(ctx, n, w, h, d2pc.DTYPE_F32, qs) as rig:
        rig.process_device(d.data_ptr(), 1.0, w * 4, h * w * 4, pts.data_ptr(), None, cap, counts.data_ptr(),
                           offsets.data_ptr(), stream())
        sec.process(pts, cap, counts=offsets[n:], stream_ptr=stream(), **out)
        torch.cuda.synchronize()
    total = int(u32(offsets)[n])
    assert 0 < total < cap
    xyz, pos = sectors_ref.gather(u32(pts)[:cap], 4, 1, cap, 0, [total])
    grid = ref.grid(xyz, pos)
    same(read_outputs(out, sec.n_cells), grid)
    seen = grid["count"] > 0
    assert grid["count"].sum() == total and 3 <= seen.sum() <= 15, "three cameras of 5 degrees each see a few sectors each"
    assert np.all(grid["distance_cm"][~seen] == 65535) and np.all(grid["distance_cm"][seen] < 65535)


def test_parity_cloud_with_inf_and_nan_points(ctx):
    """A PARITY cloud keeps its holes as non-finite points (x / 0; 0 / 0 on the principal point's column): all dropped."""
    h, w, border, f = 37, 70, 3, 2
    roi_n = (h - 2 * border) * (w - 2 * border)
    disp = disparities(f, h, w, seed=81, holes=0.5)
    disp[:, :, 35] = 0.0
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_PARITY)
    ctx.set_q(d2pc.make_q(cx=35.0, cy=18.0))
    d = torch.from_numpy(disp).to(DEV)
    pts = torch.full((f * roi_n + GUARD, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros(f, dtype=torch.int32, device=DEV)
    ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, f, pts.data_ptr(), None, roi_n, counts.data_ptr(), stream())
    sec, ref = session(r_min=0.5)
    out = fresh_outputs(sec.n_cells)
    sec.process(pts, roi_n, n_clouds=f, counts=counts, frame_stride_points=roi_n, stream_ptr=stream(), **out)
    torch.cuda.synchronize()
    ctx.check_async_error()
    ctx.set_q(d2pc.make_q())
    words = u32(pts)[:f * roi_n]
    cloud = words[:, :3].copy().view(F32)
    assert np.isinf(cloud).any() and np.isnan(cloud).any() and np.isfinite(cloud).all(axis=1).any()
    xyz, pos = sectors_ref.gather(words, 4, f, roi_n, roi_n, u32(counts))
    grid = ref.grid(xyz, pos)
    same(read_outputs(out, sec.n_cells), grid)
    assert 0 < grid["count"].sum() <= np.isfinite(cloud).all(axis=1).sum()


def test_textured_cloud_gives_the_same_grid(ctx):
    """The 32-byte records d2pc_texture_device makes of a cloud: same cells, same positions."""
    h, w, border, f = 37, 70, 3, 3
    roi_n = (h - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_COMPACT)
    d = torch.from_numpy(disparities(f, h, w, seed=91)).to(DEV)
    pts = torch.full((f * stride, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.zeros((f * stride,), dtype=torch.int32, device=DEV)
    counts = torch.zeros(f, dtype=torch.int32, device=DEV)
    ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, f, pts.data_ptr(), idx.data_ptr(), stride,
                       counts.data_ptr(), stream())
    image = torch.randint(0, 256, (f, h, w), dtype=torch.uint8, device=DEV)
    rec = torch.full((f * stride, 8), PT_SENTINEL, dtype=torch.int32, device=DEV)
    ctx.texture_device(d2pc.texture_desc_init(width=w, height=h, n_frames=f, texture=image.data_ptr(), tex_pitch=w, tex_frame_stride=h * w,
                                              points=pts.data_ptr(), index=idx.data_ptr(), counts=counts.data_ptr(), cloud_points=roi_n,
                                              points_frame_stride_points=stride, out=rec.data_ptr(), out_frame_stride_points=stride), stream())
    sec, ref = session(r_min=0.5)
    plain = run(sec, pts, roi_n, f, stride, counts, 16)
    textured = run(sec, rec, roi_n, f, stride, counts, 32)
    for k in OUTPUTS:
        assert plain[k].tobytes() == textured[k].tobytes(), k
    xyz, pos = sectors_ref.gather(u32(rec).reshape(-1, 8), 8, f, roi_n, stride, u32(counts))
    same(textured, ref.grid(xyz, pos))
    assert plain["count"].sum() > 0


# -------------------------------------------------------------------------------------------------------- addresses
def test_points_beyond_4_gib_of_an_allocation():
    """`points` (two clouds, 32-byte records) and the outputs lie past offset 2^32 of one allocation."""
    need = (1 << 32) + (64 << 20)
    if torch.cuda.mem_get_info()[0] < need + (1 << 30):
        pytest.skip("the device cannot hold the %.1f GiB of this arena" % (need / 2 ** 30))
    arena = torch.empty(need, dtype=torch.uint8, device=DEV)
    try:
        sec, ref = session(n_sectors=72, n_layers=3, u_min=-4.0, u_max=5.0, r_min=1.0, r_max=12.0)
        cp, stride = 3000, 3100
        words = records(random_xyz(2 * stride, seed=95), 32)
        G = 1 << 32
        p_off, o_off = G + 4096 + 16, G + (32 << 20)
        arena[p_off:p_off + words.nbytes] = dev_words(words).view(torch.uint8).reshape(-1)
        arena[o_off:o_off + 8192] = 0xA5
        base = arena.data_ptr()
        n = sec.n_cells
        sec.process(base + p_off, cp, point_step=32, n_clouds=2, frame_stride_points=stride, range=base + o_off,
                    count=base + o_off + 1024, nearest=base + o_off + 2048, distance_cm=base + o_off + 3072, stream_ptr=stream())
        torch.cuda.synchronize()
        raw = arena[o_off:o_off + 8192].cpu().numpy()
        grid = ref.grid(*sectors_ref.gather(words, 8, 2, cp, stride))
        got = dict(range=raw[:4 * n].view(np.uint32), count=raw[1024:1024 + 4 * n].view(np.uint32),
                   nearest=raw[2048:2048 + 4 * n].view(np.uint32), distance_cm=raw[3072:3072 + 2 * n].view(np.uint16))
        same(got, grid)
        for a, b in ((4 * n, 1024), (1024 + 4 * n, 2048), (2048 + 4 * n, 3072), (3072 + 2 * n, 8192)):
            assert np.all(raw[a:b] == 0xA5), "bytes between the outputs were written"
    finally:
        del arena
        torch.cuda.empty_cache()


# --------------------------------------------------------------------------------------------------------- refusals
def test_refusals_enqueue_nothing():
    sec, ref = session()
    words = records(random_xyz(500, seed=97))
    pts = dev_words(words)
    out = fresh_outputs(sec.n_cells)
    lib = d2pc.load_sectors_library()

    def status(**kw):
        args = dict(points=pts.data_ptr(), cloud_points=500, **{k: t.data_ptr() for k, t in out.items()})
        desc = d2pc.sectors_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_process_device(sec.handle, ctypes.byref(desc), stream())
        assert st == d2pc.sectors_desc_check(sec.cfg, desc)
        return st

    assert status(point_step=24) == 1 and "point_step" in sec.last_error()
    assert status(cloud_points=0) == 3 and status(range=pts.data_ptr() + 16) == 1 and "overlaps" in sec.last_error()
    assert status(count=out["range"].data_ptr() + 8) == 1 and status(n_clouds=2, points_frame_stride_points=499) == 3
    torch.cuda.synchronize()
    read_outputs(out, 0)           # every entry still holds its sentinel
    assert status() == 0
    torch.cuda.synchronize()
    same(read_outputs(out, sec.n_cells), ref.grid(*sectors_ref.gather(words, 4, 1, 500, 0)))
