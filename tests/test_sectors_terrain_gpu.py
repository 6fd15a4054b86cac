"""d2pc_sectors_terrain_update_device on the GPU.  Every update's count, sum, sum2, mean_q, spread_q2, flat, site, candidates,
summary and status, and the state block behind it, are compared byte for byte with tests/sectors_terrain_ref.py; every
output is sentinel-filled with guard entries behind it.  Most cases feed planted frame tables (as ground calls could have
written them), no cloud; one case is checked against an oracle that owes nothing to the reference: ONE ground call over all
the window's clouds.  tests/README_sectors_terrain.md has the map of cases."""
import ctypes

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ground_ref as gref
import sectors_ref
import sectors_terrain_ref as tref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 16
F32 = np.float32
NONE = 0xFFFFFFFFFFFFFFFF
OFF = 0xFFFFFFFF
GROUND_OUT = ("count", "sum", "sum2", "mean_q", "spread_q2", "flat", "site", "candidates", "summary")
OUT = GROUND_OUT + ("status",)
DTYPE = dict(count=np.uint32, sum=np.int64, sum2=np.uint64, mean_q=np.int32, spread_q2=np.uint32, flat=np.uint8, site=np.uint8,
             candidates=np.uint64, summary=np.uint32, status=np.uint32)
SIGNED = dict(count=np.int32, sum=np.int64, sum2=np.int64, mean_q=np.int32, spread_q2=np.int32, flat=np.uint8, site=np.uint8,
              candidates=np.int64, summary=np.int32, status=np.int32)     # (torch has no unsigned 32 / 64)
SENTINEL = dict(count=0x5A5AA5A5, sum=0x3C3CC3C35A5AA5A5, sum2=0x3C3CC3C35A5AA5A6, mean_q=0x5A5AA5A6, spread_q2=0x5A5AA5A7, flat=0xA5, site=0xA6,
                candidates=0x3C3CC3C35A5AA5A7, summary=0x7FC3C3C3, status=0x7FC3C3C4)   # no call here produces them
EYE, ZERO = np.eye(3), np.zeros(3)
GRIDS = {"2x2": dict(n_a=2, n_b=2, window=0), "5x3": dict(n_a=5, n_b=3), "16x16": dict(), "33x31": dict(n_a=33, n_b=31),
         "32x32": dict(n_a=32, n_b=32), "33x32": dict(n_a=33, n_b=32), "64x64": dict(n_a=64, n_b=64, window=2)}
# planted heights are small and spreads modest: cells are flat and sites exist
JUDGE = dict(cell_size=0.5, min_count=1, max_spread_q2=40000, max_step_q=300, w_dist=2, w_rough=1)
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
    return dict({o: n_cells for o in OUT}, candidates=k, summary=4, status=4)


def fresh_outputs(n_cells, k, want=OUT):
    size = sizes(n_cells, k)
    return {o: to_dev(np.full(size[o] + GUARD, SENTINEL[o], dtype=DTYPE[o]), SIGNED[o]) for o in want}


def read_outputs(out, n_cells, k):
    """-> the outputs as numpy; asserts the guard entries behind each."""
    size = sizes(n_cells, k)
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


def tables(rng, n, fill=0.8, k_range=150):
    """Frame tables a ground call could have written: 0 .. 5 heights of |k| <= k_range per cell -> (count, sum, sum2)."""
    per = np.where(rng.random(n) < fill, rng.integers(1, 6, n), 0)
    ks = rng.integers(-k_range, k_range + 1, (n, 5)) * (np.arange(5)[None, :] < per[:, None])
    return per.astype(np.uint32), ks.sum(axis=1).astype(np.int64), (ks * ks).sum(axis=1).astype(np.uint64)


def corner_step(ia, jb, h0=1.0, goal=(OFF, OFF), cell=0.5):
    return gref.step_words(EYE, ZERO, [cell * ia, cell * jb, h0], *goal)


class Harness:
    """A terrain session and its reference in lockstep; run() makes one update of both and compares outputs and state."""

    def __init__(self, depth, **cfg):
        self.cfg = d2pc.sectors_ground_config_init(**cfg)
        self.terrain = d2pc.SectorsTerrain(self.cfg, depth=depth)
        self.ref = tref.SectorsTerrainRef(self.cfg, d2pc.sectors_ground_geometry(self.cfg), depth)
        self.n_a, self.n_b, self.n_cells, self.depth = self.cfg.n_a, self.cfg.n_b, self.terrain.n_cells, depth
        self.step = torch.zeros(20, dtype=torch.int32, device=DEV)
        self.state = self.terrain.state_tensor()
        assert self.state.numel() == self.terrain.geometry.state_bytes == len(self.ref.state)
        self.reset()

    def close(self):
        del self.state
        self.terrain.close()

    def reset(self):
        self.terrain.reset(stream())
        self.ref.reset()

    def read_state(self):
        torch.cuda.synchronize()
        return self.state.cpu().numpy().copy()

    def plant_state(self, state):
        self.state.copy_(torch.from_numpy(np.ascontiguousarray(state, dtype=np.uint8)).to(DEV))
        self.ref.state[:] = state

    def device(self, step, frame, allowed=None, k=5, want=OUT):
        """One d2pc_sectors_terrain_update_device -> the outputs as numpy."""
        self.step.copy_(to_dev(step, np.int32))
        fc, fs, fs2 = to_dev(frame[0], np.int32), to_dev(frame[1], np.int64), to_dev(frame[2], np.int64)
        a_dev = torch.from_numpy(np.asarray(allowed, dtype=np.uint8)).to(DEV) if allowed is not None else None
        out = fresh_outputs(self.n_cells, k, want)
        self.terrain.update(self.step, fc, fs, fs2, allowed=a_dev, n_candidates=k, stream_ptr=stream(), **out)
        torch.cuda.synchronize()
        return read_outputs(out, self.n_cells, k)

    def run(self, step, frame, allowed=None, k=5, want=OUT, what=""):
        """-> the reference's result, which the device's equals bit for bit, as the state block does."""
        step = np.asarray(step, dtype=np.uint32)
        got = self.device(step, frame, allowed, k, want)
        exp = self.ref.update(step, *frame, allowed=allowed, n_candidates=k)
        same(got, exp, what)
        state = self.read_state()
        bad = np.flatnonzero(state != self.ref.state)
        assert bad.size == 0, "%s: state byte %d is %#x, not %#x (%d differ)" % (what, bad[0], state[bad[0]], self.ref.state[bad[0]], bad.size)
        return exp


def harness(depth, **cfg):
    key = (depth,) + tuple(sorted((k, tuple(v) if isinstance(v, (list, tuple)) else v) for k, v in cfg.items()))
    if key not in _made:
        _made[key] = Harness(depth, **cfg)
    h = _made[key]
    h.reset()
    return h


# ------------------------------------------------------------------------------------------------ grids x depths
@pytest.mark.parametrize("depth", [1, 2, 3, 16])
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids_and_depths_under_a_random_walk(name, depth):
    """depth + 2 updates (the ring wraps) of planted tables while the corner walks by up to two cells an update, every update
    compared.  1,023 / 1,024 / 1,025 cells lie around the lane count; 5 x 3 rounds slot_bytes up (300 -> 304)."""
    h = harness(depth, **dict(JUDGE, **GRIDS[name]))
    rng = np.random.default_rng(h.n_cells * 100 + depth)
    ia, jb, most, sites = 10, -7, 0, 0
    for it in range(depth + 2):
        ia, jb = ia + int(rng.integers(-2, 3)), jb + int(rng.integers(-2, 3))
        goal = (int(rng.integers(0, h.n_a)), int(rng.integers(0, h.n_b)))
        r = h.run(corner_step(ia, jb, goal=goal), tables(rng, h.n_cells), k=5, what="%s, depth %d, update %d" % (name, depth, it))
        assert r["status"].tolist() == [it + 1, r["status"][1], ia & OFF, jb & OFF]
        most, sites = max(most, int(r["status"][1])), sites + int(r["summary"][2])
    assert most == depth if min(h.n_a, h.n_b) >= 16 else most >= min(depth, 2) or h.n_a == 2, "the window never held what it should"
    assert sites > 0 or h.n_cells < 100, "no site was ever found: the judging did not matter"


# ------------------------------------------------------------------------------------------------ the ring
def test_ring_of_three_over_eight_updates_and_depth_one():
    h = harness(3, **dict(JUDGE, **GRIDS["5x3"]))
    rng = np.random.default_rng(8)
    frames = [tables(rng, 15, fill=1.0) for _ in range(8)]
    for it, f in enumerate(frames):
        r = h.run(corner_step(0, 0), f, what="ring update %d" % it)
        assert r["status"].tolist() == [it + 1, min(it + 1, 3), 0, 0]
        window = frames[max(0, it - 2):it + 1]
        assert np.array_equal(r["count"], sum(w[0].astype(np.int64) for w in window)) and np.array_equal(r["sum"], sum(w[1] for w in window))
        hdr = h.read_state()[:256].view(np.uint32).reshape(16, 4)
        assert int(np.argmax(hdr[:3, 3])) == it % 3 and not hdr[3:].any(), "the smallest seq is replaced; headers beyond depth stay zero"
    one = harness(1, **dict(JUDGE, **GRIDS["5x3"]))
    for it, f in enumerate(frames[:3]):
        r = one.run(corner_step(it, 0), f, what="depth 1, update %d" % it)
        assert r["status"][:2].tolist() == [it + 1, 1]
        assert np.array_equal(r["count"], f[0]) and np.array_equal(r["sum"], f[1]) and np.array_equal(r["sum2"], f[2]), "the frame alone"


# ------------------------------------------------------------------------------------------------ the scroll
def shifted_sum(n_a, n_b, new, old, di, dj):
    """new + old read at (i + di, j + dj) where that lies inside: written with slices, not with the reference's index."""
    out = new.astype(np.int64).reshape(n_b, n_a).copy()
    o = old.astype(np.int64).reshape(n_b, n_a)
    i0, i1, j0, j1 = max(0, -di), min(n_a, n_a - di), max(0, -dj), min(n_b, n_b - dj)
    if i0 < i1 and j0 < j1:
        out[j0:j1, i0:i1] += o[j0 + dj:j1 + dj, i0 + di:i1 + di]
    return out.reshape(-1)


def test_shifts_of_0_1_n_minus_1_n_and_n_plus_1_along_each_axis_and_diagonally():
    n_a, n_b = 12, 9
    h = harness(2, **dict(JUDGE, n_a=n_a, n_b=n_b))
    rng = np.random.default_rng(21)
    old, new = tables(rng, n_a * n_b, fill=1.0), tables(rng, n_a * n_b, fill=1.0)
    along_a = [0, 1, -1, n_a - 1, -(n_a - 1), n_a, -n_a, n_a + 1, -(n_a + 1)]
    along_b = [0, 1, -1, n_b - 1, -(n_b - 1), n_b, -n_b, n_b + 1, -(n_b + 1)]
    shifts = [(d, 0) for d in along_a] + [(0, d) for d in along_b[1:]] + list(zip(along_a[1:], along_b[1:])) + [(1, -1), (-(n_a - 1), n_b - 1), (n_a - 1, n_b)]
    for di, dj in shifts:
        h.reset()
        h.run(corner_step(100, -50), old, what="the older frame")
        r = h.run(corner_step(100 + di, -50 + dj, goal=(3, 4)), new, what="shift (%d, %d)" % (di, dj))
        in_sight = abs(di) < n_a and abs(dj) < n_b
        assert r["status"].tolist() == [2, 2 if in_sight else 1, 100 + di, (-50 + dj) & OFF]
        assert np.array_equal(r["count"], shifted_sum(n_a, n_b, new[0], old[0], di, dj)), (di, dj)
        assert np.array_equal(r["sum"], shifted_sum(n_a, n_b, new[1], old[1], di, dj)), (di, dj)
        assert np.array_equal(r["sum2"].astype(np.int64), shifted_sum(n_a, n_b, new[2], old[2], di, dj)), (di, dj)


def test_corners_round_half_to_even_and_anchor_up_to_2_to_the_29():
    h = harness(4, **dict(JUDGE, n_a=40, n_b=36, cell_size=1.0))
    rng = np.random.default_rng(22)
    for a0, b0, ia, jb in ((2.5, 3.5, 2, 4), (3.5, -0.5, 4, 0), (-0.5, -2.5, 0, -2), (-1.5, 0.49999997, -2, 0)):
        r = h.run(gref.step_words(EYE, ZERO, [a0, b0, 1.0]), tables(rng, h.n_cells), what="corner (%r, %r)" % (a0, b0))
        assert r["status"][2:].tolist() == [ia & OFF, jb & OFF] and r["status"][1] == r["status"][0], "the four frames overlap"
    h.reset()
    top = 536870912.0
    below = float(np.nextafter(F32(top), F32(0)))               # 2^29 - 32: a neighbour 32 cells away
    assert top - below == 32.0
    frames = [tables(rng, h.n_cells, fill=1.0) for _ in range(4)]
    r = h.run(gref.step_words(EYE, ZERO, [top, -top, 1.0]), frames[0], what="anchored at +-2^29")
    assert r["status"].tolist() == [1, 1, 1 << 29, (-(1 << 29)) & OFF]
    r = h.run(gref.step_words(EYE, ZERO, [below, -below, 1.0]), frames[1], what="the neighbour across")
    assert r["status"].tolist() == [2, 2, (1 << 29) - 32, (-(1 << 29) + 32) & OFF]
    assert np.array_equal(r["count"], shifted_sum(40, 36, frames[1][0], frames[0][0], -32, 32))
    r = h.run(gref.step_words(EYE, ZERO, [-top, top, 1.0]), frames[2], what="the opposite corner: a difference of 2^30")
    assert r["status"].tolist() == [3, 1, (-(1 << 29)) & OFF, 1 << 29]
    r = h.run(gref.step_words(EYE, ZERO, [-below, below, 1.0]), frames[3], what="its neighbour")
    assert r["status"][:2].tolist() == [4, 2]


def test_corners_beyond_the_anchor_nan_and_inf_leave_the_state_untouched():
    h = harness(3, **dict(JUDGE, **GRIDS["5x3"], cell_size=1.0))
    rng = np.random.default_rng(23)
    h.run(corner_step(0, 0, cell=1.0), tables(rng, 15, fill=1.0), what="a first frame")
    h.run(corner_step(1, 0, cell=1.0), tables(rng, 15, fill=1.0), what="a second frame")
    before = h.read_state()
    beyond = float(np.nextafter(F32(536870912.0), F32(np.inf)))
    for a0, b0 in ((beyond, 0.0), (0.0, -beyond), (np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (3e38, 3e38)):
        r = h.run(gref.step_words(EYE, ZERO, [a0, b0, 1.0], 2, 1), tables(rng, 15, fill=1.0), k=3, what="corner (%r, %r)" % (a0, b0))
        assert np.array_equal(h.read_state(), before), "a frame that is not anchored wrote the state"
        assert r["status"].tolist() == [2, 0, 0, 0] and r["summary"].tolist() == [0, 0, 0, 0] and np.all(r["candidates"] == NONE)
        assert not r["count"].any() and not r["sum"].any() and not r["sum2"].any() and not r["flat"].any() and not r["site"].any()
        assert np.all(r["mean_q"] == -(1 << 31)) and np.all(r["spread_q2"] == 0xFFFFFFFF)
    r = h.run(corner_step(1, 1, cell=1.0), tables(rng, 15, fill=1.0), what="anchored again")
    assert r["status"].tolist() == [3, 3, 1, 1]


# ------------------------------------------------------------------------------------------------ h0
def test_h0_drops_takes_up_again_signed_zeros_and_nan():
    h = harness(8, **dict(JUDGE, **GRIDS["5x3"]))
    rng = np.random.default_rng(24)
    took = []
    for h0 in (1.0, 1.0, 2.0, 1.0, 0.0, -0.0, np.nan, np.nan, -0.0, 1.0):
        r = h.run(corner_step(0, 0, h0=h0), tables(rng, 15, fill=1.0), what="h0 %r" % h0)
        took.append(int(r["status"][1]))
    # 1.0 twice; 2.0 alone; back to 1.0: three; +0.0 alone; -0.0 equals it; NaN alone, twice; -0.0: three; the last 1.0 finds one other
    # 1.0 among the eight newest frames
    assert took == [1, 2, 1, 3, 1, 2, 1, 1, 3, 2]
    hdr = h.read_state()[:256].view(np.uint32).reshape(16, 4)
    assert sorted(hdr[:8, 2].tolist()).count(0x80000000) == 2 and (hdr[:8, 2] == 0x7FC00000).sum() == 2, "h0 is stored as its bits"


# ------------------------------------------------------------------------------------------------ wrapping
def test_counts_that_wrap_and_a_state_whose_seq_is_all_ones():
    h = harness(2, **dict(JUDGE, **GRIDS["2x2"]))
    big = (np.array([0x80000000, 3, 0, 0], dtype=np.uint32), np.array([0, 30, 0, 0], dtype=np.int64), np.array([0, 300, 0, 0], dtype=np.uint64))
    h.run(corner_step(0, 0), big, what="2^31 points in a cell")
    r = h.run(corner_step(0, 0), big, what="and 2^31 more")
    assert r["count"].tolist() == [0, 6, 0, 0] and r["mean_q"].tolist() == [-(1 << 31), 10, -(1 << 31), -(1 << 31)]
    assert r["spread_q2"][0] == 0xFFFFFFFF and r["flat"].tolist() == [0, 1, 0, 0] and r["summary"][0] == 6
    # sums that wrap modulo 2^64 follow the formulas (the per-cell outputs are specified, site / candidates are not compared)
    wrap = (np.array([1, 1, 1, 1], dtype=np.uint32), np.array([-(1 << 63), 5, 0, 0], dtype=np.int64), np.array([1 << 63, 25, 0, 0], dtype=np.uint64))
    h.reset()
    h.run(corner_step(0, 0), wrap, want=("count", "sum", "sum2", "mean_q", "spread_q2", "flat", "status"), what="sums of 2^63")
    r = h.run(corner_step(0, 0), wrap, want=("count", "sum", "sum2", "mean_q", "spread_q2", "flat", "status"), what="wrapped sums")
    assert r["sum"][0] == 0 and r["sum2"][0] == 0 and r["count"][0] == 2
    # a planted state: slot 1 holds seq 0xFFFFFFFF -> all slots are first taken as empty
    d3 = harness(3, **dict(JUDGE, **GRIDS["5x3"]))
    rng = np.random.default_rng(25)
    for it in range(3):
        d3.run(corner_step(it, 0), tables(rng, 15, fill=1.0), what="filling")
    state = d3.read_state()
    state[:256].view(np.uint32).reshape(16, 4)[1, 3] = 0xFFFFFFFF
    d3.plant_state(state)
    f = tables(rng, 15, fill=1.0)
    r = d3.run(corner_step(1, 0), f, what="restart")
    assert r["status"].tolist() == [1, 1, 1, 0] and np.array_equal(r["count"], f[0])
    hdr = d3.read_state()[:256].view(np.uint32).reshape(16, 4)
    assert hdr[0].tolist() == [1, 0, F32(1.0).view(np.uint32), 1] and not hdr[1:].any()
    r = d3.run(corner_step(1, 0), f, what="after the restart")
    assert r["status"].tolist() == [2, 2, 1, 0] and np.array_equal(r["count"], 2 * f[0])
    # a planted seq of 0xFFFFFFFE steps to 0xFFFFFFFF, and the update after that restarts
    state = d3.read_state()
    state[:256].view(np.uint32).reshape(16, 4)[1, 3] = 0xFFFFFFFE
    d3.plant_state(state)
    assert d3.run(corner_step(1, 0), f, what="the last seq")["status"].tolist() == [0xFFFFFFFF, 3, 1, 0]
    assert d3.run(corner_step(1, 0), f, what="restart again")["status"].tolist() == [1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ the independent oracle
def test_three_clouds_through_ground_and_terrain_equal_one_ground_call_over_all_three():
    """Real clouds, one step: ground_process_device then terrain_update for each cloud; the window of the third update is, in
    all nine outputs and bit for bit, what ONE ground call with n_clouds = 3 gives.  No reference code takes part."""
    Q = 1.0 / 512.0
    cfg = d2pc.sectors_ground_config_init(n_a=24, n_b=20, quantum=Q, min_count=4, max_step_q=20, window=1, w_dist=3, w_rough=1)   # max_spread_q2 625
    n, k, cp, stride = 24 * 20, 7, 9000, 9100
    R64, t64, origin = gref.rotation(0.7, 0.25, -0.15), np.array([31.5, -47.25, 22.0]), np.array([28.0, -51.0, 21.0])
    rng = np.random.default_rng(26)
    world = np.stack([rng.uniform(27.5, 40.5, 3 * stride), rng.uniform(-51.5, -40.5, 3 * stride),
                      origin[2] + 100 * Q + rng.normal(0.0, 5 * Q, 3 * stride)], axis=1)
    world[rng.random(3 * stride) < 0.001, 2] += 1.0                    # a few outliers: some cells are not flat
    words = np.full((3 * stride, 4), 0x12345678, dtype=np.uint32)
    words[:, :3] = ((world - t64) @ R64).astype(F32).view(np.uint32)
    pts = to_dev(words, np.int32)
    step = to_dev(gref.step_words(R64, t64, origin, 11, 7), np.int32)
    with d2pc.SectorsGround(cfg) as ground, d2pc.SectorsTerrain(cfg, depth=3) as terrain:
        want = fresh_outputs(n, k, GROUND_OUT)
        ground.process(pts, cp, step, n_clouds=3, frame_stride_points=stride, n_candidates=k, stream_ptr=stream(), **want)
        frame = fresh_outputs(n, k, ("count", "sum", "sum2"))
        for c in range(3):
            out = fresh_outputs(n, k)
            ground.process(pts[c * stride:], cp, step, stream_ptr=stream(), **frame)
            terrain.update(step, frame["count"], frame["sum"], frame["sum2"], n_candidates=k, stream_ptr=stream(), **out)
        torch.cuda.synchronize()
        want, got = read_outputs(want, n, k), read_outputs(out, n, k)
    assert got.pop("status").tolist() == [3, 3, 56, (-102) & OFF]
    for o in GROUND_OUT:
        assert got[o].tobytes() == want[o].tobytes(), o
    assert want["summary"][0] > 15000 and 0 < want["summary"][2] < want["summary"][1] < n and want["candidates"][k - 1] != NONE
    assert want["candidates"][0] != want["candidates"][1]


# ------------------------------------------------------------------------------------------------ the state
def test_save_restore_reset_and_two_runs_give_the_same_bytes():
    h = harness(4, **dict(JUDGE, **GRIDS["16x16"]))
    rng = np.random.default_rng(27)
    frames = [tables(rng, 256) for _ in range(5)]
    steps = [corner_step(i, -i, goal=(8, 8)) for i in range(5)]

    def sequence(first, last):
        return [h.device(steps[i], frames[i], k=6) for i in range(first, last)]

    def equal(a, b):
        return all(x[o].tobytes() == y[o].tobytes() for x, y in zip(a, b) for o in OUT)

    h.terrain.reset(stream())
    run1 = sequence(0, 3)
    saved = h.state.clone()                                # one copy saves the map ...
    tail1 = sequence(3, 5)
    after = h.read_state()
    h.state.copy_(saved)                                   # ... and one restores it
    tail2 = sequence(3, 5)
    assert equal(tail1, tail2) and np.array_equal(h.read_state(), after), "restore, then the same two updates"
    assert tail1[1]["status"].tolist() == [5, 4, 4, (-4) & OFF]
    h.terrain.reset(stream())
    hdr = h.read_state()[:256]
    assert not hdr.any() and np.array_equal(h.read_state()[256:], after[256:]), "reset zeroes the headers and nothing else"
    run2 = sequence(0, 3)
    assert equal(run1, run2) and run2[0]["status"].tolist() == [1, 1, 0, 0], "reset empties the window; two runs of one sequence"
    assert run2[2]["status"][1] == 3 and run2[2]["summary"][2] > 0


# ------------------------------------------------------------------------------------------------ the outputs
def test_outputs_alone_and_together_and_refusals_enqueue_nothing():
    h = harness(3, **dict(JUDGE, **GRIDS["16x16"]))
    rng = np.random.default_rng(28)
    allowed = (rng.random(256) < 0.9).astype(np.uint8)
    for it, want in enumerate([(o,) for o in OUT] + [("count", "summary"), ("flat", "site"), ("sum", "sum2", "candidates", "status"), OUT]):
        h.run(corner_step(it % 3, it % 2, goal=(7, 9)), tables(rng, 256), allowed=allowed if it % 2 else None, k=7, want=want, what="outputs %s" % (want,))
    f = tables(rng, 256)
    fc, fs, fs2 = to_dev(f[0], np.int32), to_dev(f[1], np.int64), to_dev(f[2], np.int64)
    out = fresh_outputs(h.n_cells, 5)
    lib = d2pc.load_sectors_library()
    before = h.read_state()
    state_ptr, state_bytes = h.terrain.state()

    def status(check=True, **kw):
        args = dict(step=h.step.data_ptr(), frame_count=fc.data_ptr(), frame_sum=fs.data_ptr(), frame_sum2=fs2.data_ptr(), n_candidates=5,
                    **{o: t.data_ptr() for o, t in out.items()})
        desc = d2pc.sectors_terrain_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_terrain_update_device(h.terrain.handle, ctypes.byref(desc), stream())
        assert st != 0 and (not check or st == d2pc.sectors_terrain_desc_check(h.cfg, h.terrain.tcfg, desc))
        return st

    assert status(struct_size=124) == 1 and "d2pc_sectors_terrain_desc" in h.terrain.last_error()
    assert status(step=None) == 1 and "step" in h.terrain.last_error()
    assert status(frame_count=None) == 1 and status(frame_sum=None) == 1 and status(frame_sum2=None) == 1 and "required" in h.terrain.last_error()
    assert status(n_candidates=33) == 1 and "n_candidates" in h.terrain.last_error()
    assert status(sum=out["sum"].data_ptr() + 4) == 1 and status(frame_sum=fs.data_ptr() + 4) == 1
    assert status(count=fc.data_ptr()) == 1 and "overlaps" in h.terrain.last_error()
    assert status(flat=out["site"].data_ptr() + 8) == 1
    assert status(**{o: None for o in OUT}) == 1
    # the session's own addition: its state block
    assert status(check=False, status=state_ptr + 16) == 1 and "state" in h.terrain.last_error()
    assert status(check=False, summary=state_ptr + state_bytes - 16) == 1 and status(check=False, frame_count=state_ptr + 256) == 1
    torch.cuda.synchronize()
    read_outputs(out, 0, 0)            # every entry still holds its sentinel
    assert np.array_equal(h.read_state(), before), "a refused update wrote the state"
    h.run(corner_step(1, 1), f, what="after the refusals")


# ------------------------------------------------------------------------------- behind the producer and the ground, in a graph
def test_producer_ground_and_terrain_in_one_captured_chain():
    """d2pc_process_device (COMPACT) -> d2pc_sectors_ground_process_device -> d2pc_sectors_terrain_update_device captured once;
    three replays with new frames and a new step copied into the same device words equal the reference.  An update that
    allocated, cleared with a memset node or read on the host would break the replays."""
    hh, w, border, f = 37, 70, 3, 2
    roi_n = (hh - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    k = 5
    judge = dict(min_count=2, max_spread_q2=d2pc.sectors_ground_spread_of_std(0.002, 0.8), max_step_q=400, window=1, w_dist=2)
    h = harness(4, **judge)
    gh = gref.SectorsGroundRef(h.cfg, d2pc.sectors_ground_geometry(h.cfg))
    nadir = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])        # the optical axis looks down
    poses = [(nadir, [0.0, 0.0, 10.0], [-4.0, -4.0, 8.0], 8, 8),
             (gref.rotation(0.3, 0.05, -0.04) @ nadir, [0.4, -0.2, 10.5], [-4.0, -4.5, 8.0], 3, 12),
             (gref.rotation(-1.1, -0.06, 0.02) @ nadir, [-0.3, 0.6, 9.5], [-4.5, -3.5, 8.0], OFF, 0)]
    d = torch.zeros((f, hh, w), dtype=torch.float32, device=DEV)
    pts = torch.full((f * stride, 4), 0x7FC5A5A5, dtype=torch.int32, device=DEV)
    counts = torch.zeros((f,), dtype=torch.int32, device=DEV)
    frame = fresh_outputs(h.n_cells, k, ("count", "sum", "sum2"))
    out = fresh_outputs(h.n_cells, k)
    with d2pc.SectorsGround(h.cfg) as ground, d2pc.Context(q=d2pc.make_q(fx=40.0, fy=40.0, cx=35.0, cy=18.0), border=border, compact_algo=1,
                                                          mode=d2pc.MODE_COMPACT) as ctx:
        def chain():
            s = stream()
            ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, hh, w * 4, hh * w * 4, f, pts.data_ptr(), None, stride,
                               counts.data_ptr(), s)
            ground.process(pts, roi_n, h.step, n_clouds=f, counts=counts, frame_stride_points=stride, stream_ptr=s, **frame)
            h.terrain.update(h.step, frame["count"], frame["sum"], frame["sum2"], n_candidates=k, stream_ptr=s, **out)

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
            step = gref.step_words(*poses[i])
            part, cell, kq = gh.bin(xyz, step)
            cells = gh.cells(cell[part], kq[part])
            exp = h.ref.update(step, cells["count"], cells["sum"], cells["sum2"], n_candidates=k)
            same(got, exp, what)
            assert np.array_equal(h.read_state(), h.ref.state), what
            return exp

        ctx.reserve(w, hh, f)
        plain = []
        for i in range(3):
            feed(i)
            chain()
            torch.cuda.synchronize()
            plain.append(check(i, "plain call %d" % i))
        assert plain[2]["status"][:2].tolist() == [3, 3] and plain[2]["summary"][0] > 2000 and plain[2]["summary"][1] > 0, "the window did not matter"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):              # (the capture is global: a device allocation inside it fails the call)
            chain()
        torch.cuda.synchronize()
        h.plant_state(h.ref.state.copy())      # (a capture runs nothing; the map is the reference's in any case)
        replayed = []
        for i in (2, 0, 1):
            feed(i)
            g.replay()
            torch.cuda.synchronize()
            replayed.append(check(i, "replay of step %d" % i))
        assert replayed[2]["status"][:2].tolist() == [6, 4]
        ctx.check_async_error()
        del g
        ctx.release_graph_buffers()
