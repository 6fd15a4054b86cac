"""d2pc_sectors_slope_process_device on the GPU.  Every call's count, sum, sum2, moments, slope_a, slope_b, level_q, resid_q2,
flat, site, candidates and summary are compared byte for byte, every cell, with tests/sectors_slope_ref.py (the slopes as
their bits); every output is sentinel-filled with guard entries behind it.  The built cases assert the outcome itself beside
the reference.  tests/README_sectors_slope.md has the map of cases."""
import ctypes

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ref
import sectors_slope_ref as sref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 16
F32 = np.float32
NONE = 0xFFFFFFFFFFFFFFFF
OFF = 0xFFFFFFFF
OUT = sref.OUT
DTYPE = sref.DTYPE
SIGNED = dict(count=np.int32, sum=np.int64, sum2=np.int64, moments=np.int64, slope_a=np.int32, slope_b=np.int32, level_q=np.int32,
              resid_q2=np.int32, flat=np.uint8, site=np.uint8, candidates=np.int64, summary=np.int32)     # (torch has no unsigned 32 / 64)
SENTINEL = dict(count=0x5A5AA5A5, sum=0x3C3CC3C35A5AA5A5, sum2=0x3C3CC3C35A5AA5A6, moments=0x3C3CC3C35A5AA5A8, slope_a=0x7FC5A5A1, slope_b=0x7FC5A5A2,
                level_q=0x5A5AA5A6, resid_q2=0x5A5AA5A7, flat=0xA5, site=0xA6, candidates=0x3C3CC3C35A5AA5A7, summary=0x7FC3C3C3)   # no call here produces them
PT_SENTINEL = 0x7FC5A5A5            # a NaN: a record past a cloud's count that was read would take no part -- and count is compared
EYE, ZERO = np.eye(3), np.zeros(3)
# the built cases: cells of 0.5 (inv_c = 2) and a quantum of 2^-9 (inv_q = 512), both exact
Q = 1.0 / 512.0
GRIDS = {"5x3": dict(n_a=5, n_b=3), "16x16": dict(), "46x46": dict(n_a=46, n_b=46, window=2)}
_made = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sessions():
    yield
    for h in _made.values():
        h.close()
    _made.clear()


def stream():
    return torch.cuda.current_stream().cuda_stream


def to_dev(a, signed):
    return torch.from_numpy(np.ascontiguousarray(a).view(signed).copy()).to(DEV)


def sizes(n_cells, k):
    return dict({o: n_cells for o in OUT}, moments=7 * n_cells, candidates=k, summary=4)


def fresh_outputs(n_cells, k, want=OUT):
    size = sizes(n_cells, k)
    return {o: to_dev(np.full(size[o] + 2 * GUARD, SENTINEL[o], dtype=DTYPE[o]), SIGNED[o]) for o in want}


def pointers(out):
    """The outputs' pointers: each buffer begins GUARD entries into its tensor, so the guards lie on both sides."""
    return {o: t.data_ptr() + GUARD * t.element_size() for o, t in out.items()}


def read_outputs(out, n_cells, k):
    """-> the outputs as numpy; asserts the guard entries before and behind each."""
    size = sizes(n_cells, k)
    got = {}
    for o, t in out.items():
        a = t.cpu().numpy().view(DTYPE[o])
        s = DTYPE[o](SENTINEL[o])
        assert np.all(a[:GUARD] == s) and np.all(a[GUARD + size[o]:] == s), "%s: an entry outside the buffer was written" % o
        got[o] = a[GUARD:GUARD + size[o]].copy()
    return got


def same(got, want, what=""):
    for o, a in got.items():
        w = np.asarray(want[o]).astype(DTYPE[o])
        bad = np.flatnonzero(a != w)
        assert bad.size == 0, "%s %s: entry %d is %s, not %s (%d differ)" % (what, o, bad[0], hex(int(a[bad[0]])), hex(int(w[bad[0]])), bad.size)


def records(xyz, step_words=4):
    """float32 (n, 3) -> the records as uint32 (n, step_words); the words behind z hold a pattern no test reads."""
    xyz = np.asarray(xyz, dtype=F32).reshape(-1, 3)
    w = np.full((len(xyz), step_words), 0x12345678, dtype=np.uint32)
    w[:, :3] = xyz.view(np.uint32)
    return w


class Harness:
    """A slope session and its reference; run() makes one call of both and compares."""

    def __init__(self, sub=8, max_slope=None, **cfg):
        self.cfg = d2pc.sectors_ground_config_init(**cfg)
        self.scfg = d2pc.sectors_slope_config_init(sub=sub) if max_slope is None else d2pc.sectors_slope_config_init(sub=sub, max_slope=max_slope)
        self.slope = d2pc.SectorsSlope(self.cfg, self.scfg)
        self.ref = sref.SectorsSlopeRef(self.cfg, self.scfg, d2pc.sectors_ground_geometry(self.cfg))
        assert (self.ref.scale, self.ref.max_tilt2) == (self.slope.geometry.scale, self.slope.geometry.max_tilt2)
        self.n_a, self.n_b, self.n_cells = self.cfg.n_a, self.cfg.n_b, self.slope.n_cells
        self.step = torch.zeros(20, dtype=torch.int32, device=DEV)

    def close(self):
        self.slope.close()

    def device(self, words, step, cloud_points=None, n_clouds=1, counts=None, stride=0, allowed=None, k=5, want=OUT):
        """One d2pc_sectors_slope_process_device -> the outputs as numpy."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        cloud_points = len(words) if cloud_points is None else cloud_points
        self.step.copy_(to_dev(step, np.int32))
        pts = to_dev(words, np.int32)
        c_dev = to_dev(np.asarray(counts, dtype=np.uint32), np.int32) if counts is not None else None
        a_dev = torch.from_numpy(np.asarray(allowed, dtype=np.uint8)).to(DEV) if allowed is not None else None
        out = fresh_outputs(self.n_cells, k, want)
        self.slope.process(pts, cloud_points, self.step, point_step=4 * words.shape[1], n_clouds=n_clouds, counts=c_dev,
                           frame_stride_points=stride, allowed=a_dev, n_candidates=k, stream_ptr=stream(), **pointers(out))
        torch.cuda.synchronize()
        return read_outputs(out, self.n_cells, k)

    def run(self, words, step=None, cloud_points=None, n_clouds=1, counts=None, stride=0, allowed=None, k=5, want=OUT, what=""):
        """-> the reference's result, which the device's equals bit for bit."""
        step = sref.step_words(EYE, ZERO, ZERO) if step is None else np.asarray(step, dtype=np.uint32)
        words = np.ascontiguousarray(words, dtype=np.uint32)
        cp = len(words) if cloud_points is None else cloud_points
        got = self.device(words, step, cp, n_clouds, counts, stride, allowed, k, want)
        xyz, _ = sectors_ref.gather(words, words.shape[1], n_clouds, cp, stride, counts)
        exp = self.ref.process(xyz, step, allowed, k)
        same(got, exp, what)
        return exp


def harness(**cfg):
    key = tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in cfg.items()))
    if key not in _made:
        _made[key] = Harness(**cfg)
    return _made[key]


def built(**cfg):
    """The harness of the built cases: quantum 2^-9, min_count 1 unless given."""
    return harness(**dict(dict(quantum=Q, min_count=1), **cfg))


_clouds = {}


def pose_and_cloud(h, n, seed, spread=0.02):
    """`n` camera-frame records under a tilted pose whose world points cover the grid and a margin around it: a ground that
    slopes differently in two halves, with a step between them and noise on top.  Made once per (grid, n, seed)."""
    key = (h.n_a, h.n_b, float(h.cfg.cell_size), n, seed, spread)
    if key not in _clouds:
        rng = np.random.default_rng(seed)
        R64, t64 = sref.rotation(0.7, 0.25, -0.15), np.array([31.5, -47.25, 22.0])
        ext_a, ext_b = h.n_a * float(h.cfg.cell_size), h.n_b * float(h.cfg.cell_size)
        origin = np.array([28.0, -51.0, 21.0])
        a = rng.uniform(origin[0] - 0.1 * ext_a, origin[0] + 1.1 * ext_a, n)
        b = rng.uniform(origin[1] - 0.1 * ext_b, origin[1] + 1.1 * ext_b, n)
        left = a > origin[0] + 0.5 * ext_a
        hgt = origin[2] + np.where(left, 0.3 + 0.2 * (a - origin[0]) - 0.05 * (b - origin[1]), -0.1 + 0.4 * (b - origin[1])) + rng.normal(0.0, spread, n)
        world = np.stack([a, b, hgt], axis=1)
        xyz = ((world - t64) @ R64).astype(F32)
        _clouds[key] = (xyz, sref.step_words(R64, t64, origin, h.n_a // 2, h.n_b // 3))
    return _clouds[key]


def cell_points(i, j, us, ws, ks, sub=8, h0=0.0):
    """Records at the centres of the sub-steps (u, w) of cell (i, j) of 0.5 with heights h0 + k quanta of 2^-9."""
    us, ws, ks = np.asarray(us), np.asarray(ws), np.asarray(ks)
    a = (i + ((us + sub - 1) / 2 + 0.5) / sub) * 0.5
    b = (j + ((ws + sub - 1) / 2 + 0.5) / sub) * 0.5
    return np.stack([a, b, h0 + ks * Q], axis=1).astype(F32)


US = np.arange(-7, 8, 2)
UU, WW = [x.ravel() for x in np.meshgrid(US, US)]


# ------------------------------------------------------------------------------------------------ grids x cloud sizes
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids_and_cloud_sizes_around_the_share_seam(name):
    """5 x 3 (an odd n_cells: the slab is rounded up), 16 x 16, 46 x 46 (160,816 bytes of dynamic LDS behind the attribute, one
    block per CU); 1, 1,023, 1,024, 1,025 records and enough of them that most cells are fitted."""
    h = harness(min_count=3, max_spread_q2=400, max_step_q=200, **GRIDS[name])
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert h.slope.blocks == h.slope.geometry.blocks_per_cu * cus and h.slope.geometry.blocks_per_cu == {"5x3": 4, "16x16": 4, "46x46": 1}[name]
    n = max(3000, 8 * h.n_cells)
    xyz, step = pose_and_cloud(h, n, h.n_cells)
    for m in (1, 1023, 1024, 1025, n):
        r = h.run(records(xyz[:m]), step, k=5, what="%s, %d records" % (name, m))
    assert 0.5 * n < r["summary"][0] < n, "the gate must cut and most points must take part"
    assert r["summary"][3] > 0.5 * h.n_cells and r["summary"][1] > 0 and r["summary"][3] > r["summary"][1], "fitted cells, some flat, some steep or rough"


def test_a_session_of_one_block_walks_every_share():
    h = harness(max_points=2048, min_count=3, **GRIDS["5x3"])
    assert h.slope.blocks == 1
    xyz, step = pose_and_cloud(h, 3 * 1024 + 7, 5)
    r = h.run(records(xyz), step, what="three shares and seven records, one block")
    assert r["summary"][0] > 1500


def test_three_clouds_counts_stride_and_32_byte_records():
    h = harness(min_count=3, **GRIDS["5x3"])
    cp, stride = 1500, 1700
    xyz, step = pose_and_cloud(h, 2 * stride + cp, 77)
    for step_words in (4, 8):
        words = records(xyz, step_words)
        for c in range(3):                           # between a cloud's end and the next cloud: never read
            words[c * stride + cp:(c + 1) * stride, :3] = PT_SENTINEL
        for counts in ([0, 0xFFFFFFFF, cp + 400], [1025, 7, cp], None):
            r = h.run(words, step, cloud_points=cp, n_clouds=3, counts=counts, stride=stride, what="counts %s, %d words" % (counts, step_words))
        assert r["summary"][0] > 2000 and r["summary"][3] == 15
    r = h.run(records(xyz, 8), step, cloud_points=cp, n_clouds=3, counts=[0, 0xFFFFFFFF, 0], stride=stride, what="nothing counted")
    assert r["summary"].tolist() == [0, 0, 0, 0] and np.all(r["level_q"] == -(1 << 31)) and np.all(r["resid_q2"] == 0xFFFFFFFF)
    assert np.all(r["slope_a"] == sref.NOT_FITTED) and not r["moments"].any()


# ------------------------------------------------------------------------------------------------ built points
def test_the_exact_plane_gives_exactly_0_1875_and_minus_0_125():
    """heights h0 + q (c + 3 u - 2 w), cell_size 0.5, quantum 2^-9, P 8."""
    h = built(min_count=4, **GRIDS["5x3"])
    for c, h0 in ((100, 0.0), (-3000, 0.0), (0, 12.5)):
        xyz = cell_points(1, 2, UU, WW, c + 3 * UU - 2 * WW, h0=h0)
        got = h.device(records(xyz), sref.step_words(EYE, ZERO, [0, 0, h0]))
        cell = 2 * 5 + 1
        assert got["slope_a"].view(F32)[cell] == F32(0.1875) and got["slope_b"].view(F32)[cell] == F32(-0.125)
        assert got["resid_q2"][cell] == 0 and got["level_q"][cell] == c and got["flat"][cell] == 1 and got["count"][cell] == 64
        assert got["summary"].tolist() == [64, 1, 0, 1], "W = 1: a lone flat cell is no site"
        h.run(records(xyz), sref.step_words(EYE, ZERO, [0, 0, h0]), what="c = %d" % c)


def test_cells_that_are_not_fitted_keep_the_grounds_words():
    h = built(n_a=4, n_b=3, window=0)
    clouds = [
        cell_points(0, 0, np.full(8, 3), US, 10 + 2 * US),                      # one u: A = 0
        cell_points(1, 0, [-7, 7], [-7, 7], [5, 9]),                            # 2 points
        cell_points(2, 0, US, US, 20 + US),                                     # on the diagonal: D = 0
        cell_points(0, 1, UU, WW, np.full(64, -77)),                            # level, smooth
        cell_points(1, 1, [-7, 7, -7], [-7, -7, 7], [0, 14, -28]),              # 3 points: the smallest fit
        cell_points(2, 1, [1], [1], [123]),                                     # 1 point
    ]
    r = h.run(records(np.concatenate(clouds)), what="degenerate cells")
    assert r["fitted"].tolist() == [0, 0, 0, 0, 1, 1, 0, 0, 0, 0, 0, 0] and r["summary"].tolist() == [8 + 2 + 8 + 64 + 3 + 1, 2, 2, 2]
    assert r["level_q"][:3].tolist() == [10, 7, 20] and r["resid_q2"][:3].tolist() == [84, 4, 21] and r["flat"][:3].tolist() == [0, 0, 0]
    assert r["level_q"][4] == -77 and r["resid_q2"][4] == 0 and r["level_q"][5] == -7 and r["resid_q2"][5] == 0 and r["level_q"][6] == 123


def test_points_on_cell_and_sub_step_boundaries_and_the_gates():
    h = built(**GRIDS["5x3"])
    below = np.nextafter(F32(2.5), F32(0))           # va just below n_a = 5
    pts = [(0.0, 0.0, 0), (-0.0, 0.25, 0), (0.5, 0.5, 0), (1.0, 1.0, 0), (2.0, 1.0, 0), (2.5, 0.2, 0), (below, 0.2, 0), (0.2, 1.5, 0),
           (0.2, np.nextafter(F32(1.5), F32(0)), 0), (-1e-30, 0.2, 0), (0.2, -1e-30, 0), (np.nextafter(F32(0.5), F32(0)), 0.2, 0)]
    # every sub-step boundary of cell (1, 1), from both sides
    for s in range(8):
        e = F32(0.5 + s * 0.0625)
        pts += [(e, 0.7, 0), (np.nextafter(e, F32(0)), 0.7, 0), (0.7, e, 0), (0.7, np.nextafter(e, F32(0)), 0)]
    r = h.run(records(pts), what="boundaries")
    assert r["count"][0] == 3 and r["count"][4] == 1 and r["count"][6] >= 29
    mom = r["moments"].reshape(7, 15)
    assert mom[0, 0] == -7 - 7 + 7 and mom[1, 0] == -7 + 1 - 1, "(0, 0), (-0, 0.25) and (just below 0.5, 0.2) in cell 0"
    ned = built(axes=(1, 2, -3), **GRIDS["5x3"])
    r = ned.run(records([(10.2, -3.9, -7.0 - 3 * Q)]), sref.step_words(EYE, ZERO, [10.0, -4.0, 7.0]), what="origin and NED")
    assert r["count"][0] == 1 and r["level_q"][0] == 3 and r["moments"].reshape(7, 15)[:2, 0].tolist() == [-1, -5]


def test_nan_inf_and_the_largest_k():
    h = built(n_a=2, n_b=2, window=0)
    good = (0.25, 0.75, 5 * Q)
    pts = [good]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = list(good)
            p[axis] = bad
            pts.append(tuple(p))
    pts += [good, (3.0e38, 0.25, 0.0), (0.25, 0.25, -3.0e38)]
    r = h.run(records(pts), what="NaN and inf")
    assert r["count"].tolist() == [0, 0, 2, 0] and r["sum"][2] == 10 and r["summary"].tolist() == [2, 0, 0, 0]
    # |v| at 32,767 takes part, just past it does not; the plane through +-32767 over the cell's width is the steepest exact one
    cases = [(32767.0, True), (-32767.0, True), (32767.5, False), (-32767.5, False), (32768.0, False), (-32768.0, False)]
    for v, part in cases:
        r = h.run(records([(0.25, 0.25, v * Q)]), what="v = %r" % v)
        assert r["count"][0] == (1 if part else 0)
    xyz = cell_points(0, 0, UU, WW, np.where(UU > 0, 32767, -32767))
    r = h.run(records(xyz), what="the largest heights")
    assert r["count"][0] == 64 and r["sum2"][0] == 64 * 32767 ** 2 and r["fitted"][0] == 1 and r["flat"][0] == 0
    assert r["moments"].reshape(7, 4)[5, 0] == 32767 * 32 * 8, "suk = sum |u| * 32767"
    step = sref.step_words(EYE, [np.inf, 0, 0], ZERO)
    assert h.run(records([good, good]), step, what="a step that is not finite")["summary"].tolist() == [0, 0, 0, 0]


@pytest.mark.parametrize("sub", [2, 16])
def test_sub_of_2_and_16(sub):
    h = harness(sub=sub, min_count=3, **GRIDS["5x3"])
    xyz, step = pose_and_cloud(h, 3000, 21)
    r = h.run(records(xyz), step, what="sub %d" % sub)
    assert r["summary"][3] == 15 and np.abs(r["moments"].reshape(7, 15)[0]).max() <= (sub - 1) * r["count"].max()
    b = built(sub=sub, min_count=3, n_a=4, n_b=3)
    us = np.arange(-(sub - 1), sub, 2)
    uu, ww = [x.ravel() for x in np.meshgrid(us, us)]
    r = b.run(records(cell_points(2, 1, uu, ww, 9 + uu * (16 // sub) - 3 * ww * (16 // sub), sub=sub)), what="the exact plane, sub %d" % sub)
    assert sref.as_float(r["slope_a"])[6] == F32(0.125) and sref.as_float(r["slope_b"])[6] == F32(-0.375) and r["resid_q2"][6] == 0 and r["level_q"][6] == 9


def test_tilted_attitude_and_ned_axes():
    h = harness(axes=(2, 1, -3), min_count=3, **GRIDS["5x3"])
    xyz, step = pose_and_cloud(h, 4000, 8)
    w = step.copy()
    w[12:15] = np.array([-51.0, 28.0, -21.5], dtype=F32).view(np.uint32)      # the corner in (b, a) order, h0 above the ground in NED
    r = h.run(records(xyz), w, what="axes (2, 1, -3) under a tilted pose")
    assert r["summary"][0] > 1000 and r["summary"][3] > 5


# ------------------------------------------------------------------------------------------------ contention and order
def test_64_consecutive_records_in_one_cell_and_the_same_records_shuffled():
    """Runs of 64 consecutive records in ONE cell each (a wave's lanes all add to the same ten words), heights near the
    extremes so that suk and sum2 carry between the halves of their 64-bit words."""
    h = built()
    rng = np.random.default_rng(9)
    n = 64 * 600
    cells = np.repeat(rng.integers(0, 256, n // 64), 64)
    cells[:64 * 300] = 3 * 16 + 6                    # 300 waves' worth in one cell
    i, j = cells % 16, cells // 16
    u, w = rng.choice(US, n), rng.choice(US, n)
    k = np.where(np.arange(n) % 2 == 0, 32767, -32767) + 40 * u * (np.arange(n) % 2)
    k = np.clip(k, -32767, 32767)
    xyz = cell_points(i, j, u, w, k)
    first = h.run(records(xyz), what="runs of one cell")
    cell = 3 * 16 + 6
    assert first["count"][cell] >= 64 * 300 and first["sum2"][cell] > 1 << 44
    again = h.device(records(xyz), sref.step_words(EYE, ZERO, ZERO))
    shuffled = h.device(records(xyz[rng.permutation(n)]), sref.step_words(EYE, ZERO, ZERO))
    for o in OUT:
        assert again[o].tobytes() == shuffled[o].tobytes() == np.asarray(first[o]).astype(DTYPE[o]).tobytes(), o


def test_count_sum_sum2_are_the_bytes_of_a_ground_session():
    h = harness(min_count=3, **GRIDS["16x16"])
    xyz, step = pose_and_cloud(h, 6000, 31)
    r = h.run(records(xyz), step, what="the cloud")
    with d2pc.SectorsGround(h.cfg) as ground:
        pts, st = to_dev(records(xyz), np.int32), to_dev(step, np.int32)
        c = torch.zeros(256, dtype=torch.int32, device=DEV)
        s1, s2 = torch.zeros(256, dtype=torch.int64, device=DEV), torch.zeros(256, dtype=torch.int64, device=DEV)
        ground.process(pts, len(xyz), st, count=c, sum=s1, sum2=s2, stream_ptr=stream())
        torch.cuda.synchronize()
    assert c.cpu().numpy().tobytes() == r["count"].tobytes() and s1.cpu().numpy().tobytes() == r["sum"].tobytes()
    assert s2.cpu().numpy().tobytes() == r["sum2"].tobytes()


# ------------------------------------------------------------------------------------------------ the point of the feature
def test_a_smooth_slope_and_a_rough_level_cell_come_apart_on_the_device():
    """A smooth 15 degree slope and a level cell with noise of the same spread_q2: the ground's flat is equal for both; the
    slope session calls the first steep and smooth, the second level and rough."""
    n = 4096
    rng = np.random.default_rng(15)
    a, b = rng.uniform(0.0, 0.5, n), rng.uniform(0.0, 0.5, n)
    t15 = np.tan(np.deg2rad(15.0))
    tilt = np.stack([a, b, 1.0 + (a - 0.25) * t15], axis=1)
    rough = np.stack([a + 0.5, b, 1.0 + rng.normal(0.0, 0.5 * t15 / np.sqrt(12.0), n)], axis=1)
    xyz = np.concatenate([tilt, rough]).astype(F32)
    step = sref.step_words(EYE, ZERO, [0, 0, 1.0])
    cfg = dict(n_a=2, n_b=2, window=0, min_count=4, max_spread_q2=625)
    with d2pc.SectorsGround(d2pc.sectors_ground_config_init(**cfg)) as ground:
        pts, st = to_dev(records(xyz), np.int32), to_dev(step, np.int32)
        flat, spread = torch.zeros(4, dtype=torch.uint8, device=DEV), torch.zeros(4, dtype=torch.int32, device=DEV)
        ground.process(pts, len(xyz), st, flat=flat, spread_q2=spread, stream_ptr=stream())
        torch.cuda.synchronize()
        flat, spread = flat.cpu().numpy(), spread.cpu().numpy()
    assert flat[0] == flat[1] == 1 and abs(int(spread[0]) - int(spread[1])) < 0.1 * spread[0], "the ground cannot tell them apart"
    r = harness(max_slope=d2pc.sectors_slope_of_degrees(10.0), **cfg).run(records(xyz), step, what="max_slope of 10 degrees")
    sa, sb = sref.as_float(r["slope_a"]), sref.as_float(r["slope_b"])
    assert abs(sa[0] - t15) < 0.01 and abs(sb[0]) < 0.01 and r["resid_q2"][0] < 0.1 * spread[0] and r["flat"][0] == 0, "steep and smooth"
    assert abs(sa[1]) < 0.01 and abs(sb[1]) < 0.01 and r["resid_q2"][1] > 0.9 * spread[1] and r["flat"][1] == 1, "level and rough"
    r = harness(max_slope=d2pc.sectors_slope_of_degrees(20.0), **cfg).run(records(xyz), step, what="max_slope of 20 degrees")
    assert r["flat"][:2].tolist() == [1, 1]
    r = harness(max_slope=d2pc.sectors_slope_of_degrees(20.0), **dict(cfg, max_spread_q2=60)).run(records(xyz), step, what="a tight roughness bound")
    assert r["flat"][:2].tolist() == [1, 0], "the slope is smooth about its own plane; the rubble is not"


# ------------------------------------------------------------------------------------------------ sites and candidates
@pytest.mark.parametrize("k", [1, 32])
def test_allowed_and_1_and_32_candidates(k):
    h = built(n_a=12, n_b=9, window=1, max_step_q=7, w_dist=3, w_rough=1, min_count=3)
    pts = []
    for j in range(9):
        for i in range(12):
            c = 100 + (8 if i >= 8 else 0)                                       # a step of 8 > max_step_q between columns 7 and 8
            pts.append(cell_points(i, j, [-7, 7, -7, 7], [-7, -7, 7, 7], c + np.array([-1, 1, -1, 1]) * (i % 2)))   # odd columns slope a little
    words = records(np.concatenate(pts))
    r = h.run(words, sref.step_words(EYE, ZERO, ZERO, 5, 4), k=k, what="a plateau with a step")
    site = r["site"].reshape(9, 12)
    assert site[1:8, 1:7].all() and site[1:8, 9:11].all() and not site[:, 7:9].any() and r["summary"].tolist() == [432, 108, 56, 108]
    assert r["candidates"][0] == (0 << 32 | 4 * 12 + 5) and (k == 1 or (r["candidates"][1] == (3 << 32 | 3 * 12 + 5) and np.all(r["candidates"][:32] != NONE)))
    allowed = np.ones(108, dtype=np.uint8)
    allowed[4 * 12 + 5] = 0
    r = h.run(words, sref.step_words(EYE, ZERO, ZERO, 5, 4), allowed=allowed, k=k, what="allowed")
    assert r["site"][4 * 12 + 5] == 0 and r["candidates"][0] == (3 << 32 | 3 * 12 + 5) and r["summary"][2] == 55
    allowed[:] = 0
    allowed[[2 * 12 + 2, 6 * 12 + 10]] = 1
    r = h.run(words, sref.step_words(EYE, ZERO, ZERO, OFF, OFF), allowed=allowed, k=k, what="two sites")
    assert r["candidates"].tolist() == ([2 * 12 + 2, 6 * 12 + 10] + [NONE] * 30)[:k]


# ------------------------------------------------------------------------------------------------ the outputs
def test_outputs_alone_the_two_launch_form_and_refusals_enqueue_nothing():
    h = harness(min_count=3, **GRIDS["16x16"])
    xyz, step = pose_and_cloud(h, 5000, 12)
    words = records(xyz)
    per_cell = tuple(o for o in OUT if o not in ("site", "candidates", "summary"))
    for want in [(o,) for o in OUT] + [per_cell, ("moments", "slope_a"), ("flat", "site"), ("sum", "level_q", "candidates")]:
        h.run(words, step, k=7, want=want, what="outputs %s" % (want,))      # an output that is not asked for is not written: the others' sentinels hold
    pts = to_dev(words, np.int32)
    out = fresh_outputs(h.n_cells, 5)
    lib = d2pc.load_sectors_library()

    def status(**kw):
        args = dict(points=pts.data_ptr(), cloud_points=len(words), step=h.step.data_ptr(), n_candidates=5, **pointers(out))
        desc = d2pc.sectors_slope_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_slope_process_device(h.slope.handle, ctypes.byref(desc), stream())
        assert st == d2pc.sectors_slope_desc_check(h.cfg, h.scfg, desc) and st != 0
        return st

    assert status(struct_size=136) == 1 and "d2pc_sectors_slope_desc" in h.slope.last_error()
    assert status(points=None) == 1 and status(step=None) == 1 and "step" in h.slope.last_error()
    assert status(n_candidates=33) == 1 and "n_candidates" in h.slope.last_error()
    assert status(moments=pointers(out)["moments"] + 4) == 1 and "moments" in h.slope.last_error() and status(points=pts.data_ptr() + 8) == 1
    assert status(cloud_points=0) == 3 and status(n_clouds=2, points_frame_stride_points=10) == 3
    assert status(summary=pts.data_ptr() + 160) == 1 and "overlaps" in h.slope.last_error()
    assert status(slope_b=pointers(out)["slope_a"] + 8) == 1 and status(flat=pointers(out)["moments"] + 6 * 8 * h.n_cells) == 1
    assert status(**{o: None for o in OUT}) == 1
    torch.cuda.synchronize()
    read_outputs(out, 0, 0)            # every entry still holds its sentinel
    h.run(words, step, what="after the refusals")


# ------------------------------------------------------------------------------------- in a graph, a new pose by one copy
def test_a_captured_call_replays_with_a_new_step():
    h = harness(min_count=3, **GRIDS["16x16"])
    k = 5
    xyz, step0 = pose_and_cloud(h, 6000, 44)
    words = records(xyz)
    step1 = step0.copy()
    step1[12:15] = (step0[12:15].view(F32) + np.array([0.75, -0.5, 0.125], dtype=F32)).view(np.uint32)      # the grid's corner and h0 moved
    step1[15:17] = [3, 12]
    step2 = sref.step_words(sref.rotation(0.72, 0.22, -0.13), [31.4, -47.2, 22.1], [28.0, -51.0, 21.0], OFF, OFF)
    exp = [h.ref.process(xyz, s, None, k) for s in (step0, step1, step2)]
    assert exp[0]["slope_a"].tobytes() != exp[1]["slope_a"].tobytes() != exp[2]["slope_a"].tobytes()
    pts = to_dev(words, np.int32)
    out = fresh_outputs(h.n_cells, k)

    def call():
        h.slope.process(pts, len(words), h.step, n_candidates=k, stream_ptr=stream(), **pointers(out))

    h.step.copy_(to_dev(step0, np.int32))
    call()                                       # (warm: the first launch of a kernel may load its code object)
    torch.cuda.synchronize()
    same(read_outputs(out, h.n_cells, k), exp[0], "plain call")
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):                    # (the capture is global: a device allocation or a host read inside it fails the call)
        call()
    torch.cuda.synchronize()
    for i in (1, 2, 0, 1):
        h.step.copy_(to_dev((step0, step1, step2)[i], np.int32))         # one 80-byte copy
        g.replay()
        torch.cuda.synchronize()
        same(read_outputs(out, h.n_cells, k), exp[i], "replay with step %d" % i)
    del g
