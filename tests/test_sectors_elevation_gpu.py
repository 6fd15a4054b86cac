"""d2pc_sectors_process_device with elevation layers (layer_kind = 1) on the GPU.  As in tests/test_sectors_gpu.py, whose
helpers this file uses: the clouds are crafted in device memory, the expected cells come from the numpy restatement
(tests/sectors_elev_ref.py) with the library's own tables, every comparison is of bit patterns, every output is
sentinel-filled with guard entries behind it.  tests/README_sectors_elevation.md has the map of cases."""
import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_elev_ref
import sectors_ref
import test_sectors_gpu as base

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

F32 = np.float32
OUTPUTS = base.OUTPUTS
HALF_PI = float(F32(np.pi / 2))              # 1.5707964f
INF = float("inf")
BODY = dict(axes=(1, 2, 3), r_min=0.0)       # x forward, y left, z up: f, l, u = x, y, z
# the three bands of the boundary cases: (u_min, u_max, n_layers)
BANDS = [(-HALF_PI, HALF_PI, 30), (-0.5, 0.7, 7), (-1.5707964, 1.5707964, 64)]

_sessions = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sessions():
    yield
    for sec, _ in _sessions.values():
        sec.close()
    _sessions.clear()


def session(**kw):
    """(Sectors, its reference) of a configuration, made once per module; elevation layers unless layer_kind says height."""
    kw.setdefault("layer_kind", d2pc.LAYERS_ELEVATION)
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in kw.items()))
    if key not in _sessions:
        sec = d2pc.Sectors(**kw)
        table = d2pc.sectors_table(sec.cfg)
        if kw["layer_kind"] == d2pc.LAYERS_ELEVATION:
            ref = sectors_elev_ref.SectorsElevRef(sec.cfg, table, sec.geometry, d2pc.sectors_elevation_table(sec.cfg))
        else:
            ref = sectors_ref.SectorsRef(sec.cfg, table, sec.geometry)
        _sessions[key] = (sec, ref)
    return _sessions[key]


def run(sec, points, cloud_points, n_clouds=1, stride=0, counts=None, step=16, want=OUTPUTS):
    """One call on a device tensor of records -> the outputs asked for, as numpy bit patterns (guards checked)."""
    return base.run(sec, points, cloud_points, n_clouds, stride, counts, step, want)


def check(sec, ref, words, cloud_points, n_clouds=1, stride=0, counts=None, step=16, want=OUTPUTS, what=""):
    """Upload `words` (records x step / 4 uint32), run, compare with the reference over the records the call visits."""
    words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, step // 4)
    d_counts = base.dev_words(np.asarray(counts, dtype=np.uint32)) if counts is not None else None
    got = run(sec, base.dev_words(words), cloud_points, n_clouds, stride, d_counts, step, want)
    xyz, pos = sectors_ref.gather(words, step // 4, n_clouds, cloud_points, stride, counts)
    grid = ref.grid(xyz, pos)
    base.same(got, grid, what)
    return grid


def bits(v):
    return int(np.array([v], dtype=F32).view(np.uint32)[0])


def points_in_cells(ref, cfg, cells, seed, lo=1.0, hi=12.0):
    """A point well inside each of the given cells of a BODY-axes elevation grid, in the given order, at Euclidean ranges
    lo .. hi."""
    rng = np.random.default_rng(seed)
    cells = np.asarray(cells)
    sector, layer = cells % ref.n, cells // ref.n
    theta = cfg.azimuth0 + (sector + rng.uniform(0.2, 0.8, size=len(cells))) * (2 * np.pi / ref.n)
    e = sectors_elev_ref.boundary_elevations(cfg.u_min, cfg.u_max, ref.layers)
    phi = e[0] + (layer + rng.uniform(0.2, 0.8, size=len(cells))) * ((e[-1] - e[0]) / ref.layers)
    r = rng.uniform(lo, hi, size=len(cells))
    return np.stack([r * np.cos(phi) * np.cos(theta), r * np.cos(phi) * np.sin(theta), r * np.sin(phi)], axis=1).astype(F32)


# ------------------------------------------------------------------------------------------------------------ seams
@pytest.mark.parametrize("grid", ["8x3", "60x30"])
def test_record_counts_across_the_seams_of_wave_block_and_share(grid):
    """1 .. 257 records (a wave, a block) and a share of 1,024 records -1 / +0 / +1.  8 x 3 = 24 cells take the wave's
    pre-reduction (at most 72 cells), 60 x 30 the per-lane LDS atomics alone.  One cloud in memory, cells() once, every
    prefix reduced on its own."""
    if grid == "8x3":
        sec, ref = session(n_sectors=8, n_layers=3, u_min=-0.5, u_max=0.7, r_max=15.0, **BODY)
    else:
        sec, ref = session(n_sectors=60, n_layers=30, u_min=-HALF_PI, u_max=HALF_PI, r_max=15.0, **BODY)
    assert sec.geometry.share_points == 1024 and (ref.n_cells <= 72) == (grid == "8x3")
    most = 1025
    xyz = base.random_xyz(most, seed=101)
    pts = base.dev_words(base.records(xyz))
    part, cell, d2 = ref.cells(xyz)
    assert part.sum() > most // 4 and (~part).sum() > 50          # the band and r_max drop some
    pos = np.arange(most, dtype=np.uint32)
    for n in list(range(1, 258)) + [1023, 1024, 1025]:
        base.same(run(sec, pts, n), ref.reduce(part[:n], cell[:n], d2[:n], pos[:n]), "n=%d" % n)


# ------------------------------------------------------------------------------------------------------- boundaries
def boundary_points(ref):
    """(f, l, u) = (+-ce_i 2^k, 0, se_i 2^k) for every boundary i (sqrtf(f f) = |f| exactly: the point lies ON the
    boundary as far as float32 can say), the same through the l axis, the neighbours one ulp of u either side, and
    u = +-0 with f of either sign."""
    f, l, u = [], [], []
    for scale in (F32(0.125), F32(1.0), F32(32.0)):
        c, s = ref.ce * scale, ref.se * scale                          # (a power of two: exact)
        for du in (-1, 0, 1):
            uu = s if du == 0 else np.nextafter(s, F32(du) * F32(np.inf))
            for sign in (F32(1.0), F32(-1.0)):
                f += [c * sign, np.zeros_like(c)]
                l += [np.zeros_like(c), c * sign]
                u += [uu, uu]
    f.append(np.array([3.0, 3.0, -3.0, -3.0, 1e-15, -1e-15], dtype=F32))
    l.append(np.zeros(6, dtype=F32))
    u.append(np.array([0.0, -0.0, 0.0, -0.0, -0.0, 0.0], dtype=F32))
    return base.from_flu(BODY["axes"], *(np.concatenate(v).astype(F32) for v in (f, l, u)))


@pytest.mark.parametrize("u_min,u_max,n_layers", BANDS, ids=["pi/2x30", "-0.5..0.7x7", "1.5707964x64"])
def test_boundaries(u_min, u_max, n_layers):
    sec, ref = session(n_sectors=4, n_layers=n_layers, u_min=u_min, u_max=u_max, azimuth0=-np.pi / 4, r_max=INF, **BODY)
    xyz = boundary_points(ref)
    part, cell, _ = ref.cells(xyz)
    assert part.any() and (~part).any(), "the band's own two boundaries are gates: points either side of them"
    assert set(np.unique(cell[part] // 4)) == set(range(n_layers)), "every layer has a point on or next to its boundary"
    assert set(np.unique(cell[part] % 4)) == {0, 1, 2, 3}
    check(sec, ref, base.records(xyz), len(xyz))
    grid = check(sec, ref, base.records(xyz[::-1]), len(xyz), what="reversed")
    assert grid["count"].sum() == part.sum()
    # one point per call where a point sits exactly on a boundary: a wrong bin cannot hide behind a right count
    on = np.flatnonzero(np.isin(xyz[:, 2].view(np.uint32), (ref.se * F32(32.0)).view(np.uint32)))[:2 * (n_layers + 1)]
    for i in on[:: max(1, len(on) // 8)]:
        check(sec, ref, base.records(xyz[i:i + 1]), 1, what="point %d alone" % i)


# ------------------------------------------------------------------------------------------------------------ gates
def on_sphere(d2_bits, seed, tries=4000):
    """(f, l, u) float32 triples with u != 0, at elevations of 0.2 .. 0.45 rad, whose fl(fl(fl(f f) + fl(l l)) + fl(u u))
    has exactly the given bit pattern."""
    rng = np.random.default_rng(seed)
    target = float(np.array([d2_bits], dtype=np.uint32).view(F32)[0])
    phi, theta = rng.uniform(0.2, 0.45, size=tries), rng.uniform(0, 2 * np.pi, size=tries)
    f = (np.sqrt(target) * np.cos(phi) * np.cos(theta)).astype(F32)
    l = (np.sqrt(target) * np.cos(phi) * np.sin(theta)).astype(F32)
    r2 = f * f + l * l
    u0 = np.sqrt(np.maximum(target - r2.astype(np.float64), 0)).astype(F32)
    found = []
    for step in range(-6, 7):
        u = (u0.view(np.int32) + step).astype(np.int32).view(F32)
        hit = (r2 + u * u).view(np.uint32) == d2_bits
        found.append(np.stack([f[hit], l[hit], u[hit]], axis=1))
    found = np.concatenate(found)
    assert len(found) >= 3, "no point found on the sphere"
    return found[:8]


def test_range_gate_is_on_the_euclidean_d2():
    """d2 with exactly the bit patterns of rmin2, rmax2 and their neighbours: in the horizontal plane (u = 0: d2 = r2) and
    at an elevation inside the band, where r2 alone would pass or fail differently."""
    sec, ref = session(n_sectors=72, n_layers=7, u_min=-0.5, u_max=0.7, azimuth0=0.3, axes=(1, 2, 3), r_min=0.5, r_max=25.0)
    g = sec.geometry
    assert (g.rmin2, g.rmax2) == (0.25, 625.0)
    lo, hi = bits(g.rmin2), bits(g.rmax2)
    xyz = []
    for b in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
        fl = base.on_circle(b, seed=b & 0xFFFF)
        for u in (0.0, -0.0):
            xyz.append(base.from_flu((1, 2, 3), fl[:, 0], fl[:, 1], np.full(len(fl), u)))
        xyz.append(on_sphere(b, seed=b & 0xFFF))
    xyz.append(np.array([[0.5, 0, 0], [25, 0, 0], [0, 0.4, 0.3], [20, 0, 15], [20, 0, 15.000002], [24.9, 0, 3.0]], dtype=F32))
    xyz = np.concatenate(xyz)
    part, cell, d2 = ref.cells(xyz)
    for b, inside in ((lo - 1, False), (lo, True), (lo + 1, True), (hi - 1, True), (hi, True), (hi + 1, False)):
        at = d2.view(np.uint32) == b
        assert at.sum() >= 6 and np.all(part[at] == inside), hex(b)
    # r2 = 616.01 passes a horizontal gate of 625; d2 = 634.01 does not
    assert not part[-1] and F32(24.9) * F32(24.9) <= g.rmax2
    grid = check(sec, ref, base.records(xyz), len(xyz))
    assert grid["count"].sum() == part.sum()


def test_gates_without_bounds():
    """r_min = 0 and r_max = +inf, the band +-1.5707964 x 30 (its boundary 15 is at elevation exactly 0: ce 1, se 0)."""
    sec, ref = session(n_sectors=4, n_layers=30, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 4, r_max=INF, **BODY)
    assert (ref.ce[15], ref.se[15]) == (1.0, 0.0)
    xyz = np.array([
        [0.0, 0.0, 2.0], [-0.0, 0.0, -2.0], [1e-30, -1e-30, 1.0],      # 0-2: r2 = 0 with u != 0 (the last by underflow): dropped
        [2.0 ** -70, 0.0, 0.0],                                        # 3: a subnormal r2 = d2 = 2^-140, h = 2^-70: takes part
        [0.0, 2.0 ** -70, 2.0 ** -70],                                 # 4: subnormal r2 and d2 = 2^-139, elevation pi / 4
        [-(2.0 ** -74), 0.0, -0.0],                                    # 5: r2 = 2^-148
        [1.5e19, 0.0, 1.5e19],                                         # 6: r2 is finite, d2 overflows: takes part, range +inf
        [0.0, -1.5e19, -1.9e19],                                       # 7: the same below the horizon
        [1e30, 1.0, 1.0],                                              # 8: r2 and h overflow: t_15 = 1 u - 0 inf is NaN ...
        [-1e30, 1.0, -1.0],                                            # 9: ... and takes no part in the count: layer 14
        [3e38, 1e38, 3e38], [0.0, 5.0, 0.0]], dtype=F32)               # 10: the cell of 8, and d2 = +inf as well; 11
    bad = np.tile(np.array([[2.0, 1.0, 0.5]], dtype=F32), (3 * len(base.SPECIAL), 1))      # NaNs and +-inf in x, y, z
    for i, b in enumerate(np.tile(base.SPECIAL, 3)):
        bad[i, i // len(base.SPECIAL)] = np.array([b], dtype=np.uint32).view(F32)[0]
    xyz = np.concatenate([xyz, bad])
    part, cell, d2 = ref.cells(xyz)
    assert part[:12].tolist() == [False] * 3 + [True] * 9 and not part[12:].any()
    assert cell[3:12].tolist() == [15 * 4 + 0, 22 * 4 + 1, 15 * 4 + 2, 22 * 4 + 0, 6 * 4 + 3, 14 * 4 + 0, 14 * 4 + 2, 14 * 4 + 0, 15 * 4 + 1]        # (sector 1 is left, 2 behind)
    assert np.isinf(d2[[6, 7, 8, 9, 10]]).all() and d2[3] == F32(2.0 ** -140) and d2[4] == F32(2.0 ** -139)
    grid = check(sec, ref, base.records(xyz), len(xyz))
    assert grid["count"].sum() == 9 and grid["count"][56] == 2 and grid["nearest"][56] == 8      # equal d2 (+inf): the smaller position
    assert np.isinf(grid["range"][[88, 27, 56, 58]]).all() and grid["distance_cm"][[88, 27, 56, 58]].tolist() == [65534] * 4
    assert grid["range"][60] == F32(2.0 ** -70) and grid["range"][62] == F32(2.0 ** -74) and grid["distance_cm"][60] == 0
    assert grid["range"][89] == np.sqrt(F32(2.0 ** -139)) and grid["nearest"][89] == 4


@pytest.mark.parametrize("band", [(0.0, 0.3), (-0.3, 0.0)], ids=["floor at 0", "ceiling at 0"])
def test_an_infinite_h_against_a_gate_at_elevation_zero(band):
    """h = +inf against the band's own boundary at elevation exactly 0 (se = 0: 0 inf is NaN).  Written `t_0 >= 0` and
    `not (t_n >= 0)`: a NaN t_0 keeps the point out, a NaN t_n lets it in."""
    sec, ref = session(n_sectors=4, n_layers=1, u_min=band[0], u_max=band[1], azimuth0=-np.pi / 4, r_max=INF, **BODY)
    zero = 0 if band[0] == 0.0 else 1
    assert (ref.ce[zero], ref.se[zero]) == (1.0, 0.0)
    xyz = np.array([[1e30, 1.0, 1.0], [1e30, 1.0, -1.0], [-2e30, 1e25, 1e20], [-2e30, 1e25, -1e20], [5.0, 0.0, 0.5], [0.0, 5.0, -0.5],
                    [5.0, 0.0, 0.0], [5.0, 0.0, -0.0]], dtype=F32)
    part = ref.cells(xyz)[0]
    assert part.tolist() == ([False] * 4 + [True, False, True, True] if zero == 0 else [True] * 4 + [False, True, False, False])
    grid = check(sec, ref, base.records(xyz), len(xyz))
    assert grid["count"].sum() == part.sum()


# ------------------------------------------------------------------------------------------------------------ sizes
@pytest.mark.parametrize("n_sectors,n_layers", [(60, 30), (2, 64), (90, 64)])
def test_one_point_per_cell(n_sectors, n_layers):
    """60 x 30 (the planner's histogram), 2 x 64 (the most layers on the fewest sectors) and 90 x 64: the largest table,
    69,120 + 360 + 520 bytes of dynamic LDS, beyond the 64 KB a launch gets without asking."""
    sec, ref = session(n_sectors=n_sectors, n_layers=n_layers, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / n_sectors, r_max=15.0, **BODY)
    if (n_sectors, n_layers) == (90, 64):
        assert sec.geometry.lds_bytes == 70000 and sec.geometry.blocks_per_cu == 2
    cells = np.random.default_rng(123).permutation(ref.n_cells)
    xyz = points_in_cells(ref, sec.cfg, cells, seed=124)
    part, got_cells, _ = ref.cells(xyz)
    assert part.all() and np.array_equal(got_cells, cells), "the pattern is not the one that was meant"
    grid = check(sec, ref, base.records(xyz), len(xyz))
    assert np.all(grid["count"] == 1) and np.array_equal(grid["nearest"], np.argsort(cells))
    check(sec, ref, base.records(base.random_xyz(6000, seed=125, spread=3.0)), 6000, what="random")


# ---------------------------------------------------------------------------------------------------------- layouts
HISTOGRAM = dict(n_sectors=60, n_layers=30, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60, axes=(1, 2, 3), r_min=0.2, r_max=15.0)


@pytest.mark.parametrize("step", [16, 32])
@pytest.mark.parametrize("n_clouds", [1, 3])
def test_record_and_cloud_layouts(step, n_clouds):
    sec, ref = session(**HISTOGRAM)
    cp, stride = 2500, 2500 + 37
    words = base.records(base.random_xyz(n_clouds * stride, seed=step + n_clouds), step, seed=3)
    grid = check(sec, ref, words, cp, n_clouds, stride, None, step)
    assert (grid["count"] > 0).sum() > 500 and 0 < grid["count"].sum() < n_clouds * cp
    top = int(grid["nearest"][grid["count"] > 0].max())
    assert top < cp if n_clouds == 1 else top >= 2 * stride          # a position counts the stride


def test_counts_null_ragged_clamped_failed_and_zero():
    sec, ref = session(**HISTOGRAM)
    cp, stride = 1500, 1600
    words = base.records(base.random_xyz(3 * stride, seed=111))
    check(sec, ref, words, cp, 3, stride, None)
    check(sec, ref, words, cp, 3, stride, [5, 1500, 777], what="ragged")
    check(sec, ref, words, cp, 3, stride, [1501, 0xFFFFFFFE, 1 << 31], what="clamped")
    check(sec, ref, words, cp, 3, stride, [0xFFFFFFFF, 9, 0xFFFFFFFF], what="failure mark")
    grid = check(sec, ref, words, cp, 3, stride, [0, 0xFFFFFFFF, 0], what="empty")
    assert np.isinf(grid["range"]).all() and not grid["count"].any() and np.all(grid["nearest"] == 0xFFFFFFFF)
    assert np.all(grid["distance_cm"] == 65535)


@pytest.mark.parametrize("min_count", [1, 3])
def test_outputs_alone_and_together_and_min_count(min_count):
    sec, ref = session(n_sectors=8, n_layers=3, u_min=-0.5, u_max=0.7, azimuth0=-np.pi / 8, min_count=min_count, no_obstacle_cm=3001, **BODY)
    # cells with 1, 2, 3 and 6 points; the first 24 points are the nearest of their cells
    cells = np.concatenate([np.arange(24), np.arange(0, 24, 2), np.arange(0, 24, 4), np.repeat(np.arange(0, 24, 8), 3)])
    xyz = points_in_cells(ref, sec.cfg, cells, seed=142)
    xyz[24:] *= F32(2.0 ** 21)          # (a power of two: the direction is unchanged) everything else lies behind them
    radii = np.array([2.995, 7.995, 655.33, 655.34, 655.35, 700.0, 1e6, 0.004], dtype=F32)
    xyz[:24] *= (radii[np.arange(24) % len(radii)] / np.sqrt((xyz[:24].astype(np.float64) ** 2).sum(axis=1))).astype(F32)[:, None]
    part, got_cells, _ = ref.cells(xyz)
    assert part.all() and np.array_equal(got_cells, cells)
    words = base.records(xyz)
    grid = check(sec, ref, words, len(xyz))
    assert set(grid["count"].tolist()) == {1, 2, 3, 6} and (grid["distance_cm"] == 65534).any() and np.array_equal(grid["nearest"], np.arange(24))
    masked = grid["count"] < min_count
    assert (~masked).any() and masked.any() == (min_count > 1)
    assert np.isinf(grid["range"][masked]).all() and np.all(grid["distance_cm"][masked] == 3001)
    pts = base.dev_words(words)
    for k in OUTPUTS:
        base.same(run(sec, pts, len(xyz), want=(k,)), grid, "alone")
    base.same(run(sec, pts, len(xyz), want=("range", "distance_cm")), grid, "two")


# ------------------------------------------------------------------------------------------------------ determinism
def test_same_bytes_again_and_alternating_with_a_height_session():
    """The same call twice; then a height-mode session and the elevation session take turns on one stream: each keeps its
    bytes (they share a kernel template, not a table)."""
    sec, ref = session(**HISTOGRAM)
    height, href = session(layer_kind=d2pc.LAYERS_HEIGHT, n_sectors=60, n_layers=3, u_min=-4.0, u_max=5.0, azimuth0=-np.pi / 60,
                           axes=(1, 2, 3), r_min=0.2, r_max=15.0)
    n = 3 * 1024 + 77
    words = base.records(base.random_xyz(n, seed=151))
    a = base.dev_words(words)
    xyz, pos = sectors_ref.gather(words, 4, 1, n, 0)
    want_e, want_h = ref.grid(xyz, pos), href.grid(xyz, pos)
    first = run(sec, a, n)
    second = run(sec, a, n)
    h1 = run(height, a, n)
    third = run(sec, a, n)
    h2 = run(height, a, n)
    for k in OUTPUTS:
        assert first[k].tobytes() == second[k].tobytes() == third[k].tobytes(), k
        assert h1[k].tobytes() == h2[k].tobytes(), k
    base.same(first, want_e, "elevation")
    base.same(h1, want_h, "height")
    # without a synchronisation between them: four calls queued on the stream, read at the end
    outs = [base.fresh_outputs(s.n_cells) for s in (sec, height, sec, height)]
    for s, o in zip((sec, height, sec, height), outs):
        s.process(a, n, stream_ptr=base.stream(), **o)
    torch.cuda.synchronize()
    for s, o, want in zip((sec, height, sec, height), outs, (want_e, want_h, want_e, want_h)):
        base.same(base.read_outputs(o, s.n_cells), want, "queued")
    assert want_e["count"].sum() > n // 2 and want_h["count"].sum() > n // 4


# ------------------------------------------------------------------------------------------ behind the producer
def test_one_chain_behind_the_producer():
    """d2pc_process_device (COMPACT, a 96 x 96 frame) and the elevation session on one stream, nothing between them; the
    reference runs over the producer's cloud.  A camera's optical frame: the default axes {+3, -1, -2}."""
    h = w = 96
    border, f = 3, 1
    roi_n = (h - 2 * border) * (w - 2 * border)
    sec, ref = session(n_sectors=60, n_layers=30, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60, r_min=0.2, r_max=INF)
    with d2pc.Context(q=d2pc.make_q(cx=48.0, cy=48.0), border=border, compact_algo=1) as ctx:
        ctx.set_mode(d2pc.MODE_COMPACT)
        d = torch.from_numpy(base.disparities(f, h, w, seed=161)).to(base.DEV)
        pts = torch.full((roi_n, 4), base.PT_SENTINEL, dtype=torch.int32, device=base.DEV)
        counts = torch.zeros((f,), dtype=torch.int32, device=base.DEV)
        out = base.fresh_outputs(sec.n_cells)
        s = base.stream()
        ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, f, pts.data_ptr(), None, roi_n, counts.data_ptr(), s)
        sec.process(pts, roi_n, counts=counts, stream_ptr=s, **out)
        torch.cuda.synchronize()
        ctx.check_async_error()
    cn = base.u32(counts)
    assert 0 < cn[0] < roi_n
    xyz, pos = sectors_ref.gather(base.u32(pts).reshape(-1, 4), 4, 1, roi_n, 0, cn)
    grid = ref.grid(xyz, pos)
    base.same(base.read_outputs(out, sec.n_cells), grid)
    seen = grid["count"] > 0
    assert grid["count"].sum() > roi_n // 4 and 4 <= seen.sum() < ref.n_cells // 2, "a camera sees a patch of the sphere"
