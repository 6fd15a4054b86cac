"""d2pc_sectors_ground_process_device on the GPU.  Every call's count, sum, sum2, mean_q, spread_q2, flat, site, candidates
and summary are compared byte for byte with tests/sectors_ground_ref.py; every output is sentinel-filled with guard entries
behind it.  The built cases assert the outcome itself beside the reference.  tests/README_sectors_ground.md has the map of
cases."""
import ctypes

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ground_ref as gref
import sectors_ref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 16
F32 = np.float32
NONE = 0xFFFFFFFFFFFFFFFF
OFF = 0xFFFFFFFF
OUT = ("count", "sum", "sum2", "mean_q", "spread_q2", "flat", "site", "candidates", "summary")
DTYPE = dict(count=np.uint32, sum=np.int64, sum2=np.uint64, mean_q=np.int32, spread_q2=np.uint32, flat=np.uint8, site=np.uint8,
             candidates=np.uint64, summary=np.uint32)
SIGNED = dict(count=np.int32, sum=np.int64, sum2=np.int64, mean_q=np.int32, spread_q2=np.int32, flat=np.uint8, site=np.uint8,
              candidates=np.int64, summary=np.int32)     # (torch has no unsigned 32 / 64)
SENTINEL = dict(count=0x5A5AA5A5, sum=0x3C3CC3C35A5AA5A5, sum2=0x3C3CC3C35A5AA5A6, mean_q=0x5A5AA5A6, spread_q2=0x5A5AA5A7, flat=0xA5, site=0xA6,
                candidates=0x3C3CC3C35A5AA5A7, summary=0x7FC3C3C3)   # no call here produces them
PT_SENTINEL = 0x7FC5A5A5            # a NaN: a record past a cloud's count that was read would take no part -- and count is compared
EYE, ZERO = np.eye(3), np.zeros(3)
# the built cases: cells of 0.5 (inv_c = 2) and a quantum of 2^-9 (inv_q = 512), both exact
Q = 1.0 / 512.0
GRIDS = {"2x2": dict(n_a=2, n_b=2, window=0), "5x3": dict(n_a=5, n_b=3), "16x16": dict(), "64x64": dict(n_a=64, n_b=64, window=2)}
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


def fresh_outputs(n_cells, k, want=OUT):
    size = dict({o: n_cells for o in OUT}, candidates=k, summary=4)
    return {o: to_dev(np.full(size[o] + GUARD, SENTINEL[o], dtype=DTYPE[o]), SIGNED[o]) for o in want}


def read_outputs(out, n_cells, k):
    """-> the outputs as numpy; asserts the guard entries behind each."""
    size = dict({o: n_cells for o in OUT}, candidates=k, summary=4)
    got = {}
    for o, t in out.items():
        a = t.cpu().numpy().view(DTYPE[o])
        assert np.all(a[size[o]:] == DTYPE[o](SENTINEL[o])), "%s: an entry past its end was written" % o
        got[o] = a[:size[o]].copy()
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
    """A ground session and its reference; run() makes one call of both and compares."""

    def __init__(self, **cfg):
        self.cfg = d2pc.sectors_ground_config_init(**cfg)
        self.ground = d2pc.SectorsGround(self.cfg)
        self.ref = gref.SectorsGroundRef(self.cfg, self.ground.geometry)
        self.n_a, self.n_b, self.n_cells = self.cfg.n_a, self.cfg.n_b, self.ground.n_cells
        self.step = torch.zeros(20, dtype=torch.int32, device=DEV)

    def close(self):
        self.ground.close()

    def device(self, words, step, cloud_points=None, n_clouds=1, counts=None, stride=0, allowed=None, k=5, want=OUT):
        """One d2pc_sectors_ground_process_device -> the outputs as numpy."""
        words = np.ascontiguousarray(words, dtype=np.uint32)
        cloud_points = len(words) if cloud_points is None else cloud_points
        self.step.copy_(to_dev(step, np.int32))
        pts = to_dev(words, np.int32)
        c_dev = to_dev(np.asarray(counts, dtype=np.uint32), np.int32) if counts is not None else None
        a_dev = torch.from_numpy(np.asarray(allowed, dtype=np.uint8)).to(DEV) if allowed is not None else None
        out = fresh_outputs(self.n_cells, k, want)
        self.ground.process(pts, cloud_points, self.step, point_step=4 * words.shape[1], n_clouds=n_clouds, counts=c_dev,
                            frame_stride_points=stride, allowed=a_dev, n_candidates=k, stream_ptr=stream(), **out)
        torch.cuda.synchronize()
        return read_outputs(out, self.n_cells, k)

    def run(self, words, step=None, cloud_points=None, n_clouds=1, counts=None, stride=0, allowed=None, k=5, want=OUT, what=""):
        """-> the reference's result, which the device's equals bit for bit."""
        step = gref.step_words(EYE, ZERO, ZERO) if step is None else np.asarray(step, dtype=np.uint32)
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


def pose_and_cloud(h, n, seed, spread=0.05):
    """`n` camera-frame records under a tilted pose whose world points cover the grid and a margin around it, heights around
    a plane with a step in it."""
    rng = np.random.default_rng(seed)
    R64, t64 = gref.rotation(0.7, 0.25, -0.15), np.array([31.5, -47.25, 22.0])
    ext_a, ext_b = h.n_a * float(h.cfg.cell_size), h.n_b * float(h.cfg.cell_size)
    origin = np.array([28.0, -51.0, 21.0])
    a = rng.uniform(origin[0] - 0.1 * ext_a, origin[0] + 1.1 * ext_a, n)
    b = rng.uniform(origin[1] - 0.1 * ext_b, origin[1] + 1.1 * ext_b, n)
    hgt = origin[2] + np.where(a > origin[0] + 0.5 * ext_a, 0.3, -0.1) + rng.normal(0.0, spread, n)
    world = np.stack([a, b, hgt], axis=1)
    xyz = ((world - t64) @ R64).astype(F32)
    return xyz, gref.step_words(R64, t64, origin, h.n_a // 2, h.n_b // 3)


def key_of(cost, cell):
    return (int(cost) << 32) | int(cell)


# ------------------------------------------------------------------------------------------------ grids x cloud sizes
@pytest.mark.parametrize("name", list(GRIDS))
@pytest.mark.parametrize("max_points", [0, 2048], ids=["by-device", "one-block"])
def test_grids_and_cloud_sizes_around_the_share_and_lane_seams(name, max_points):
    """1 .. 2 x 1,024 + 7 records of a tilted pose.  max_points 2048 gives a session of ONE block, which walks the three
    shares of the largest cloud: a call larger than max_points stays correct."""
    h = harness(max_points=max_points, **GRIDS[name])
    assert h.ground.blocks == (1 if max_points else h.ground.geometry.blocks_per_cu * torch.cuda.get_device_properties(0).multi_processor_count)
    xyz, step = pose_and_cloud(h, 2 * 1024 + 7, h.n_cells)
    took = 0
    for n in (1, 255, 256, 1023, 1024, 1025, 2 * 1024 + 7):
        r = h.run(records(xyz[:n]), step, k=5, what="%s, %d records" % (name, n))
        took = int(r["summary"][0])
    assert 0.5 * 2055 < took < 2055, "the gate must cut and most points must take part"


def test_three_clouds_counts_stride_and_32_byte_records():
    h = harness(**GRIDS["5x3"])
    cp, stride = 1500, 1700
    xyz, step = pose_and_cloud(h, 2 * stride + cp, 77)
    for step_words in (4, 8):
        words = records(xyz, step_words)
        for c in range(3):                           # between a cloud's end and the next cloud: never read
            words[c * stride + cp:(c + 1) * stride, :3] = PT_SENTINEL
        for counts in ([0, 0xFFFFFFFF, cp + 400], [1025, 7, cp], [cp, cp, cp], None):
            r = h.run(words, step, cloud_points=cp, n_clouds=3, counts=counts, stride=stride, what="counts %s, %d words" % (counts, step_words))
        assert r["summary"][0] > 2000
        # one cloud of the same buffer: the stride is ignored
        h.run(words, step, cloud_points=cp, n_clouds=1, counts=[1400], stride=0, what="one cloud")
    r = h.run(records(xyz, 8), step, cloud_points=cp, n_clouds=3, counts=[0, 0xFFFFFFFF, 0], stride=stride, what="nothing counted")
    assert r["summary"].tolist() == [0, 0, 0, 0] and np.all(r["mean_q"] == -(1 << 31)) and np.all(r["spread_q2"] == 0xFFFFFFFF)


# ------------------------------------------------------------------------------------------------ built points
def test_points_on_cell_boundaries_and_the_gates_of_a_and_b():
    h = built(**GRIDS["5x3"])
    below = np.nextafter(F32(2.5), F32(0))           # va just below n_a = 5
    pts = [(0.0, 0.0, 0), (-0.0, 0.25, 0), (0.5, 0.5, 0), (1.0, 1.0, 0), (2.0, 1.0, 0), (2.5, 0.2, 0), (below, 0.2, 0), (0.2, 1.5, 0),
           (0.2, np.nextafter(F32(1.5), F32(0)), 0), (-1e-30, 0.2, 0), (0.2, -1e-30, 0), (np.nextafter(F32(0.5), F32(0)), 0.2, 0)]
    r = h.run(records(pts), what="boundaries")
    want = np.zeros(15, dtype=np.uint32)
    for cell in (0, 0, 1 * 5 + 1, 2 * 5 + 2, 2 * 5 + 4, 4, 2 * 5 + 0, 0):
        want[cell] += 1
    assert np.array_equal(r["count"], want), "va = -0.0 and an integer va take part in the cell they begin; va = n_a does not"
    # a transposed index would put (ia, ib) = (4, 0) into cell 12
    r = h.run(records([(2.2, 0.1, 0)]), what="5 x 3 is not 3 x 5")
    assert r["count"][4] == 1 and r["count"].sum() == 1
    # the grid's corner moved by the step's origin; NED picks
    ned = built(axes=(1, 2, -3), **GRIDS["5x3"])
    r = ned.run(records([(10.2, -3.9, -7.0 - 3 * Q)]), gref.step_words(EYE, ZERO, [10.0, -4.0, 7.0]), what="origin and NED")
    assert r["count"][0] == 1 and r["mean_q"][0] == 3


def test_height_gate_rounding_half_to_even_and_the_largest_k():
    h = built(**GRIDS["2x2"])
    cases = [(32767.0, 32767), (-32767.0, -32767), (32767.5, None), (-32767.5, None), (32768.0, None), (-32768.0, None),
             (0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (32766.5, 32766), (-32766.5, -32766), (0.49999997, 0)]
    for v, k in cases:
        r = h.run(records([(0.25, 0.25, v * Q)]), what="v = %r" % v)
        assert F32(v * Q) * F32(512.0) == F32(v), "the built height is exact"
        if k is None:
            assert r["count"][0] == 0 and r["summary"][0] == 0
        else:
            assert (r["count"][0], r["sum"][0], r["sum2"][0], r["mean_q"][0], r["spread_q2"][0]) == (1, k, k * k, k, 0), v
    r = h.run(records([(0.25, 0.25, v * Q) for v, k in cases]), what="all in one cell")
    ks = [k for _, k in cases if k is not None]
    assert r["count"][0] == len(ks) and r["sum"][0] == sum(ks) and r["sum2"][0] == sum(k * k for k in ks)


def test_nan_and_inf_in_each_coordinate_and_a_pose_that_overflows():
    h = built(**GRIDS["2x2"])
    good = (0.25, 0.75, 5 * Q)
    pts = [good]
    for bad in (np.nan, np.inf, -np.inf):
        for axis in range(3):
            p = list(good)
            p[axis] = bad
            pts.append(tuple(p))
    pts += [good, (3.0e38, 0.25, 0.0), (0.25, 0.25, -3.0e38)]
    r = h.run(records(pts), what="NaN and inf")
    assert r["count"].tolist() == [0, 0, 2, 0] and r["sum"][2] == 10 and r["summary"][0] == 2
    # R[0] * x overflows to +inf (and R[3] * x with R[4] * y to inf - inf = NaN): the record takes no part
    R = np.array([[3.0e38, 0, 0], [3.0e38, -3.0e38, 0], [0, 0, 1.0]])
    r = h.run(records([(4.0, 4.0, 0.0), (0.0, 0.0, 0.0), (1e-37, 0.0, 0.0)]), gref.step_words(R, ZERO, ZERO), what="a pose that overflows")
    assert r["count"].tolist() == [1, 0, 0, 0], "(0, 0, 0) alone: the third record lands at a = 30"
    # a translation that is infinite, a NaN origin: nothing takes part
    for step in (gref.step_words(EYE, [np.inf, 0, 0], ZERO), gref.step_words(EYE, ZERO, [0, np.nan, 0]), gref.step_words(EYE, ZERO, [0, 0, np.inf])):
        r = h.run(records([good, good]), step, what="a step that is not finite")
        assert r["summary"].tolist() == [0, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ contention
def test_one_cell_300000_records_alternating_extremes_and_shuffled():
    """Every record in ONE cell, k = +-32767 alternating: sum cancels, sum2 = 300,000 x 32767^2 passes 2^48, so a lost carry
    between the words of the 64-bit add shows.  The same cloud shuffled gives the same bytes."""
    h = built()
    n = 300_000
    rng = np.random.default_rng(9)
    xyz = np.zeros((n, 3), dtype=F32)
    xyz[:, 0], xyz[:, 1] = rng.uniform(3.0, 3.49, n), rng.uniform(1.5, 1.99, n)        # cell (6, 3)
    k = np.where(np.arange(n) % 2 == 0, 32767, -32767)
    xyz[:, 2] = (k * Q).astype(F32)
    r = h.run(records(xyz), what="one cell")
    cell = 3 * 16 + 6
    assert r["count"][cell] == n and r["sum"][cell] == 0 and r["sum2"][cell] == n * 32767 ** 2 > 1 << 48
    assert r["mean_q"][cell] == 0 and r["spread_q2"][cell] == 32767 ** 2 and r["count"].sum() == n
    first = h.device(records(xyz), gref.step_words(EYE, ZERO, ZERO))
    again = h.device(records(xyz[rng.permutation(n)]), gref.step_words(EYE, ZERO, ZERO))
    for o in OUT:
        assert first[o].tobytes() == again[o].tobytes(), o
    r = h.run(records(xyz[:n - 1]), what="an odd number")
    assert r["sum"][cell] == 32767 and r["mean_q"][cell] == 0
    r = h.run(records(xyz[1:]), what="an odd number, the other way")
    assert r["sum"][cell] == -32767 and r["mean_q"][cell] == -1, "floor division towards -inf"


def test_producer_order_and_shuffled_give_the_same_bytes():
    h = harness()
    xyz, step = pose_and_cloud(h, 60_000, 4, spread=0.03)
    order = np.lexsort((xyz[:, 0], np.floor(xyz[:, 1] * 8)))           # rows of neighbouring records, as a camera makes them
    first = h.run(records(xyz[order]), step, k=32, what="producer order")
    got = h.device(records(xyz[np.random.default_rng(1).permutation(len(xyz))]), step, k=32)
    for o in OUT:
        assert got[o].tobytes() == np.asarray(first[o]).astype(DTYPE[o]).tobytes(), o
    assert first["summary"][1] > 100 and first["summary"][2] > 10


# ------------------------------------------------------------------------------------------------ sites
def cloud_of_cells(h, heights, per_cell=1):
    """`per_cell` records in the middle of every cell whose entry of `heights` (k, n_b x n_a) is not None."""
    pts = []
    for j in range(h.n_b):
        for i in range(h.n_a):
            k = heights[j][i]
            if k is not None:
                pts += [((i + 0.5) * 0.5, (j + 0.5) * 0.5, k * Q)] * per_cell
    return records(pts)


def test_a_plateau_with_a_hole_steps_the_edge_allowed_and_the_goal():
    h = built(n_a=12, n_b=9, window=1, max_step_q=7, w_dist=3, w_rough=1)
    flat = [[100] * 12 for _ in range(9)]
    r = h.run(cloud_of_cells(h, flat), gref.step_words(EYE, ZERO, ZERO, 5, 4), k=5, what="a plateau over the whole grid")
    site = r["site"].reshape(9, 12)
    assert site[1:8, 1:11].all() and site.sum() == 7 * 10, "a plateau touching the edge: no site within W of it"
    assert r["candidates"].tolist() == [key_of(0, 4 * 12 + 5), key_of(3, 3 * 12 + 5), key_of(3, 4 * 12 + 4), key_of(3, 4 * 12 + 6), key_of(3, 5 * 12 + 5)]
    assert r["summary"].tolist() == [108, 108, 70, 0]
    hole = [row[:] for row in flat]
    hole[4][5] = None
    r = h.run(cloud_of_cells(h, hole), gref.step_words(EYE, ZERO, ZERO, 5, 4), k=5, what="a one-cell hole")
    site = r["site"].reshape(9, 12)
    assert not site[3:6, 4:7].any() and site.sum() == 70 - 9 and r["candidates"][0] == key_of(3 * 4, 2 * 12 + 5)
    for dk, level in ((7, True), (8, False), (-7, True), (-8, False)):
        stepped = [[100 + (dk if i >= 6 else 0) for i in range(12)] for _ in range(9)]
        r = h.run(cloud_of_cells(h, stepped), what="a step of %d" % dk)
        site = r["site"].reshape(9, 12)
        assert site[1:8, 5:7].all() == level and not (site[1:8, 5:7].any() and not level), dk
        assert site[1:8, 1:5].all() and site[1:8, 7:11].all()
    # allowed masks the best site; a goal index >= n switches the distance off
    allowed = np.ones(108, dtype=np.uint8)
    allowed[4 * 12 + 5] = 0
    r = h.run(cloud_of_cells(h, flat), gref.step_words(EYE, ZERO, ZERO, 5, 4), allowed=allowed, k=5, what="allowed")
    assert r["site"][4 * 12 + 5] == 0 and r["candidates"][0] == key_of(3, 3 * 12 + 5) and r["summary"][2] == 69
    for goal in ((12, 4), (5, 9), (OFF, OFF)):
        r = h.run(cloud_of_cells(h, flat), gref.step_words(EYE, ZERO, ZERO, *goal), k=5, what="goal %s" % (goal,))
        assert r["candidates"].tolist() == [key_of(0, 12 + 1 + c) for c in range(5)], "one cost everywhere: the smallest cells"
    # roughness: two records 10 quanta apart in one cell cost w_rough * 25 more
    rough = cloud_of_cells(h, flat)
    extra = records([((5 + 0.5) * 0.5, (4 + 0.5) * 0.5, 110 * Q)])
    r = h.run(np.concatenate([rough, extra]), gref.step_words(EYE, ZERO, ZERO, 5, 4), k=1, what="roughness")
    assert r["spread_q2"][4 * 12 + 5] == 25 and r["mean_q"][4 * 12 + 5] == 105 and r["candidates"][0] == key_of(3, 3 * 12 + 5)


@pytest.mark.parametrize("k", [1, 5, 32])
def test_fewer_sites_than_candidates(k):
    h = built(n_a=12, n_b=9, window=1, max_step_q=7, w_dist=3, w_rough=1)
    heights = [[None] * 12 for _ in range(9)]
    for j in range(0, 3):
        for i in range(2, 6):
            heights[j][i] = 40                       # 4 x 3 cells at the grid's edge: the sites (3, 1) and (4, 1)
    for j in range(5, 8):
        for i in range(8, 11):
            heights[j][i] = -40                      # 3 x 3: the site (9, 6)
    r = h.run(cloud_of_cells(h, heights, 2), gref.step_words(EYE, ZERO, ZERO, 9, 6), k=k, what="K = %d" % k)
    want = [key_of(0, 6 * 12 + 9), key_of(3 * (25 + 25), 12 + 4), key_of(3 * (36 + 25), 12 + 3)]
    assert r["candidates"].tolist() == (want + [NONE] * 32)[:k] and r["summary"].tolist() == [42, 21, 3, 0]
    h0 = built(n_a=12, n_b=9, window=0, max_step_q=7, w_dist=3, w_rough=1, min_count=3)
    r = h0.run(cloud_of_cells(h0, heights, 2), k=k, what="min_count 3: nothing is flat")
    assert np.all(r["candidates"] == NONE) and r["summary"].tolist() == [42, 0, 0, 0]


def test_the_largest_grid_more_cells_than_the_sites_block_has_lanes():
    h = built(**GRIDS["64x64"])
    heights = [[(i * 7 + j * 3) % 5 for i in range(64)] for j in range(64)]
    for goal in ((63, 63), (0, 0), (31, 40), (63, 15), (OFF, 0)):
        r = h.run(cloud_of_cells(h, heights), gref.step_words(EYE, ZERO, ZERO, *goal), k=32, what="goal %s" % (goal,))
        assert r["summary"].tolist() == [4096, 4096, 60 * 60, 0]
    allowed = np.zeros(4096, dtype=np.uint8)
    allowed[[61 * 64 + 61, 61 * 64 + 60, 2 * 64 + 2, 1023, 1024 + 64 + 2]] = 1        # 1023 lies within W of the edge
    r = h.run(cloud_of_cells(h, heights), gref.step_words(EYE, ZERO, ZERO, 61, 61), allowed=allowed, k=5, what="sites in the last lanes")
    assert [int(c) & 0xFFFFFFFF for c in r["candidates"]] == [61 * 64 + 61, 61 * 64 + 60, 1024 + 64 + 2, 2 * 64 + 2, NONE & 0xFFFFFFFF]
    wide = built(n_a=64, n_b=64, window=8, max_step_q=65535, w_dist=4095, w_rough=4095, rough_cap=65535)
    r = wide.run(cloud_of_cells(wide, heights), gref.step_words(EYE, ZERO, ZERO, 0, 0), k=32, what="W = 8")
    assert r["summary"][2] == 48 * 48 and r["candidates"][0] == key_of(4095 * 128, 8 * 64 + 8)
    small = built(n_a=16, n_b=16, window=8)
    r = small.run(cloud_of_cells(small, [[0] * 16] * 16), what="a window wider than the grid")
    assert r["summary"].tolist() == [256, 256, 0, 0] and np.all(r["candidates"] == NONE)


@pytest.mark.parametrize("goal", [(2, 50), (OFF, OFF)], ids=["goal-on-the-last", "goal-off"])
def test_one_lane_of_the_sites_block_holds_every_winner_in_a_row(goal):
    """The only allowed cells are (2, 2), (2, 18), (2, 34) and (2, 50): 130, 1,154, 2,178 and 3,202, which lane 130 of the
    sites' block holds in its slots 0 .. 3 (W = 2: i = 2 is no border cell), so one lane wins round after round and looks
    for its next key each time; with the goal on the last of them its best key sits in its last slot."""
    h = built(**GRIDS["64x64"])
    heights = [[(i * 7 + j * 3) % 5 for i in range(64)] for j in range(64)]
    cells = [130, 1154, 2178, 3202]
    allowed = np.zeros(4096, dtype=np.uint8)
    allowed[cells] = 1
    r = h.run(cloud_of_cells(h, heights), gref.step_words(EYE, ZERO, ZERO, *goal), allowed=allowed, k=5, what="goal %s" % (goal,))
    got = [int(c) & 0xFFFFFFFF for c in r["candidates"][:4]]
    assert got == (cells[::-1] if goal[0] != OFF else cells) and r["candidates"][4] == NONE and r["summary"][2] == 4


# ------------------------------------------------------------------------------------------------ the outputs
def test_outputs_alone_and_together_and_refusals_enqueue_nothing():
    h = harness()
    xyz, step = pose_and_cloud(h, 5000, 12)
    words = records(xyz)
    for want in [(o,) for o in OUT] + [("count", "summary"), ("flat", "site"), ("sum", "sum2", "candidates"), OUT]:
        h.run(words, step, k=7, want=want, what="outputs %s" % (want,))
    pts = to_dev(words, np.int32)
    out = fresh_outputs(h.n_cells, 5)
    lib = d2pc.load_sectors_library()

    def status(**kw):
        args = dict(points=pts.data_ptr(), cloud_points=len(words), step=h.step.data_ptr(), n_candidates=5, **{o: t.data_ptr() for o, t in out.items()})
        desc = d2pc.sectors_ground_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_ground_process_device(h.ground.handle, ctypes.byref(desc), stream())
        assert st == d2pc.sectors_ground_desc_check(h.cfg, desc) and st != 0
        return st

    assert status(struct_size=132) == 1 and "d2pc_sectors_ground_desc" in h.ground.last_error()
    assert status(points=None) == 1 and status(step=None) == 1 and "step" in h.ground.last_error()
    assert status(n_candidates=33) == 1 and "n_candidates" in h.ground.last_error()
    assert status(sum=out["sum"].data_ptr() + 4) == 1 and status(points=pts.data_ptr() + 8) == 1
    assert status(cloud_points=0) == 3 and status(n_clouds=2, points_frame_stride_points=10) == 3
    assert status(summary=pts.data_ptr() + 160) == 1 and "overlaps" in h.ground.last_error()
    assert status(flat=out["site"].data_ptr() + 8) == 1
    assert status(**{o: None for o in OUT}) == 1
    torch.cuda.synchronize()
    read_outputs(out, 0, 0)            # every entry still holds its sentinel
    h.run(words, step, what="after the refusals")


# ------------------------------------------------------------------------------------- behind the producer, in a graph
def test_producer_and_ground_in_one_captured_chain():
    """d2pc_process_device (COMPACT) -> d2pc_sectors_ground_process_device captured once; three replays with new frames and a
    new step copied into the same device words equal the reference for that step.  A call that allocated, or a pose kept on
    the host, would break the replays."""
    hh, w, border, f = 37, 70, 3, 2
    roi_n = (hh - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    k = 5
    h = harness(min_count=2, max_spread_q2=d2pc.sectors_ground_spread_of_std(0.002, 0.8), max_step_q=400, window=1, w_dist=2)
    nadir = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])        # the optical axis looks down
    poses = [(nadir, [0.0, 0.0, 10.0], [-4.0, -4.0, 8.0], 8, 8),
             (gref.rotation(0.3, 0.05, -0.04) @ nadir, [0.4, -0.2, 10.5], [-4.0, -4.5, 8.5], 3, 12),
             (gref.rotation(-1.1, -0.06, 0.02) @ nadir, [-0.3, 0.6, 9.5], [-4.5, -3.5, 7.5], OFF, 0)]
    d = torch.zeros((f, hh, w), dtype=torch.float32, device=DEV)
    pts = torch.full((f * stride, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros((f,), dtype=torch.int32, device=DEV)
    out = fresh_outputs(h.n_cells, k)
    with d2pc.Context(q=d2pc.make_q(fx=40.0, fy=40.0, cx=35.0, cy=18.0), border=border, compact_algo=1, mode=d2pc.MODE_COMPACT) as ctx:
        def chain():
            s = stream()
            ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, hh, w * 4, hh * w * 4, f, pts.data_ptr(), None, stride,
                               counts.data_ptr(), s)
            h.ground.process(pts, roi_n, h.step, n_clouds=f, counts=counts, frame_stride_points=stride, n_candidates=k, stream_ptr=s, **out)

        def feed(i):
            rng = np.random.default_rng(90 + i)
            disp = rng.uniform(1.5, 3.0, size=(f, hh, w)).astype(F32)
            disp[rng.random(size=disp.shape) < 0.3] = 0.0
            d.copy_(torch.from_numpy(disp))
            h.step.copy_(to_dev(gref.step_words(*poses[i]), np.int32))

        def check(i, what):
            got = read_outputs(out, h.n_cells, k)
            words = pts.cpu().numpy().view(np.uint32).reshape(-1, 4)
            xyz, _ = sectors_ref.gather(words, 4, f, roi_n, stride, counts.cpu().numpy().view(np.uint32))
            exp = h.ref.process(xyz, gref.step_words(*poses[i]), None, k)
            same(got, exp, what)
            return exp

        ctx.reserve(w, hh, f)
        plain = []
        for i in range(3):
            feed(i)
            chain()
            torch.cuda.synchronize()
            plain.append(check(i, "plain call %d" % i))
        assert plain[0]["summary"][0] > 1000 and plain[0]["summary"][1] > 0, "the ground did not matter"
        assert plain[0]["count"].tobytes() != plain[1]["count"].tobytes()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):              # (the capture is global: a device allocation inside it fails the call)
            chain()
        torch.cuda.synchronize()
        for i in (2, 0, 1):
            feed(i)
            g.replay()
            torch.cuda.synchronize()
            check(i, "replay of step %d" % i)
        ctx.check_async_error()
        del g
        ctx.release_graph_buffers()
