"""d2pc_sectors_relief_update_device on the GPU.  Every update's thirteen outputs, and the state block behind it, are compared
byte for byte with tests/sectors_relief_ref.py; every output is sentinel-filled with guard entries behind it.  Most cases feed
planted frame tables (tests/sectors_relief_cases.py: per-cell point sets on a synthetic world, as slope calls could have
written them), no cloud; one case is checked against an oracle that owes nothing to the reference: ONE slope call over all the
window's clouds.  tests/README_sectors_relief.md has the map of cases."""
import ctypes

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ground_ref as gref
import sectors_ref
import sectors_relief_cases as cases
import sectors_relief_ref as rref
import sectors_slope_ref as sref

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 16
F32 = np.float32
NONE = 0xFFFFFFFFFFFFFFFF
OFF = 0xFFFFFFFF
SLOPE_OUT = sref.OUT
OUT = rref.OUT
DTYPE = rref.DTYPE
SIGNED = dict(count=np.int32, sum=np.int64, sum2=np.int64, moments=np.int64, slope_a=np.int32, slope_b=np.int32, level_q=np.int32, resid_q2=np.int32,
              flat=np.uint8, site=np.uint8, candidates=np.int64, summary=np.int32, status=np.int32)     # (torch has no unsigned 32 / 64)
SENTINEL = dict(count=0x5A5AA5A5, sum=0x3C3CC3C35A5AA5A5, sum2=0x3C3CC3C35A5AA5A6, moments=0x3C3CC3C35A5AA5A8, slope_a=0x7FC5A5A5, slope_b=0x7FC5A5A6,
                level_q=0x5A5AA5A6, resid_q2=0x5A5AA5A7, flat=0xA5, site=0xA6, candidates=0x3C3CC3C35A5AA5A7, summary=0x7FC3C3C3,
                status=0x7FC3C3C4)   # no call here produces them
FRAME = ("count", "sum", "sum2", "moments")
GRIDS = {"2x2": dict(n_a=2, n_b=2, window=0), "5x3": dict(n_a=5, n_b=3, window=0), "4x4": dict(n_a=4, n_b=4, window=0), "6x3": dict(n_a=6, n_b=3, window=0),
         "33x31": dict(n_a=33, n_b=31), "32x32": dict(n_a=32, n_b=32), "25x41": dict(n_a=25, n_b=41), "46x46": dict(n_a=46, n_b=46),
         "64x32": dict(n_a=64, n_b=32)}
JUDGE = cases.JUDGE
corner_step = cases.corner_step
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
    return dict({o: n_cells for o in OUT}, moments=7 * n_cells, candidates=k, summary=4, status=4)


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
        w = np.ascontiguousarray(want[o]).view(DTYPE[o]) if np.asarray(want[o]).dtype.itemsize == np.dtype(DTYPE[o]).itemsize else np.asarray(want[o]).astype(DTYPE[o])
        bad = np.flatnonzero(a != w)
        assert bad.size == 0, "%s %s: entry %d is %s, not %s (%d differ)" % (what, o, bad[0], hex(int(a[bad[0]])), hex(int(w[bad[0]])), bad.size)


def frame_to_dev(frame):
    return [to_dev(frame[0], np.int32), to_dev(frame[1], np.int64), to_dev(frame[2], np.int64), to_dev(frame[3], np.int64)]


class Harness:
    """A relief session and its reference in lockstep; run() makes one update of both and compares outputs and state."""

    def __init__(self, depth, sub=8, max_slope=0.26794919, **cfg):
        self.cfg = d2pc.sectors_ground_config_init(**cfg)
        self.scfg = d2pc.sectors_slope_config_init(sub=sub, max_slope=max_slope)
        self.relief = d2pc.SectorsRelief(self.cfg, self.scfg, depth=depth)
        self.ref = rref.SectorsReliefRef(self.cfg, self.scfg, d2pc.sectors_ground_geometry(self.cfg), depth)
        self.n_a, self.n_b, self.n_cells, self.depth = self.cfg.n_a, self.cfg.n_b, self.relief.n_cells, depth
        assert (self.relief.geometry.scale, self.relief.geometry.max_tilt2) == (self.ref.slope.scale, self.ref.slope.max_tilt2)
        assert self.relief.blocks == (self.n_cells + 15) // 16
        self.step = torch.zeros(20, dtype=torch.int32, device=DEV)
        self.state = self.relief.state_tensor()
        assert self.state.numel() == self.relief.geometry.state_bytes == len(self.ref.state)
        self.reset()

    def close(self):
        del self.state
        self.relief.close()

    def reset(self):
        self.relief.reset(stream())
        self.ref.reset()

    def read_state(self):
        torch.cuda.synchronize()
        return self.state.cpu().numpy().copy()

    def plant_state(self, state):
        self.state.copy_(torch.from_numpy(np.ascontiguousarray(state, dtype=np.uint8)).to(DEV))
        self.ref.state[:] = state

    def device(self, step, frame, allowed=None, k=5, want=OUT):
        """One d2pc_sectors_relief_update_device -> the outputs as numpy."""
        self.step.copy_(to_dev(step, np.int32))
        a_dev = torch.from_numpy(np.asarray(allowed, dtype=np.uint8)).to(DEV) if allowed is not None else None
        out = fresh_outputs(self.n_cells, k, want)
        self.relief.update(self.step, *frame_to_dev(frame), allowed=a_dev, n_candidates=k, stream_ptr=stream(), **out)
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


# ------------------------------------------------------------------------------------------------ 1. grids x depths
@pytest.mark.parametrize("depth", [1, 2, 3, 16])
@pytest.mark.parametrize("name", list(GRIDS))
def test_grids_and_depths_under_a_random_walk(name, depth):
    """depth + 2 updates (the ring wraps) of planted tables while the corner walks by up to two cells an update, every update
    compared.  15 cells round slot_bytes up (1,140 -> 1,152); 16 fill one block and 18 two; 1,023 / 1,024 / 1,025 lie around a
    block seam; the last block of 46 x 46 holds 4 cells."""
    h = harness(depth, **dict(JUDGE, **GRIDS[name]))
    rng = np.random.default_rng(h.n_cells * 100 + depth)
    ia, jb, most, fitted, flat, sites, unfit = 10, -7, 0, 0, 0, 0, 0
    for it in range(depth + 2):
        ia, jb = ia + int(rng.integers(-2, 3)), jb + int(rng.integers(-2, 3))
        goal = (int(rng.integers(0, h.n_a)), int(rng.integers(0, h.n_b)))
        r = h.run(corner_step(ia, jb, goal=goal), cases.frame_tables(rng, h.n_a, h.n_b, ia, jb), k=5, what="%s, depth %d, update %d" % (name, depth, it))
        assert r["status"].tolist() == [it + 1, r["status"][1], ia & OFF, jb & OFF]
        most = max(most, int(r["status"][1]))
        fitted, flat, sites = fitted + int(r["summary"][3]), flat + int(r["summary"][1]), sites + int(r["summary"][2])
        unfit += int(((r["count"] > 0) & ~r["fitted"]).sum())
    assert most == depth if min(h.n_a, h.n_b) >= 25 else most >= min(depth, 2) or h.n_a == 2, "the window never held what it should"
    assert fitted > 0 and flat > 0 and sites > 0, "no cell was ever fitted, flat and a site: the judging did not matter"
    assert fitted > flat > 0 or h.n_cells < 100, "no fitted cell was ever refused as steep or rough"
    assert unfit > 0 or h.n_cells < 100, "no cell with points was ever left unfitted"


# ------------------------------------------------------------------------------------------------ 2. the scroll
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
    n = n_a * n_b
    h = harness(2, **dict(JUDGE, n_a=n_a, n_b=n_b))
    rng = np.random.default_rng(21)
    along_a = [0, 1, -1, n_a - 1, -(n_a - 1), n_a, -n_a, n_a + 1, -(n_a + 1)]
    along_b = [0, 1, -1, n_b - 1, -(n_b - 1), n_b, -n_b, n_b + 1, -(n_b + 1)]
    shifts = [(d, 0) for d in along_a] + [(0, d) for d in along_b[1:]] + list(zip(along_a[1:], along_b[1:])) + [(1, -1), (-(n_a - 1), n_b - 1), (n_a - 1, n_b)]
    for di, dj in shifts:
        h.reset()
        old, new = cases.frame_tables(rng, n_a, n_b, 100, -50, fill=1.0), cases.frame_tables(rng, n_a, n_b, 100 + di, -50 + dj, fill=1.0)
        h.run(corner_step(100, -50), old, what="the older frame")
        r = h.run(corner_step(100 + di, -50 + dj, goal=(3, 4)), new, what="shift (%d, %d)" % (di, dj))
        in_sight = abs(di) < n_a and abs(dj) < n_b
        assert r["status"].tolist() == [2, 2 if in_sight else 1, 100 + di, (-50 + dj) & OFF]
        assert np.array_equal(r["count"], shifted_sum(n_a, n_b, new[0], old[0], di, dj)), (di, dj)
        assert np.array_equal(r["sum"], shifted_sum(n_a, n_b, new[1], old[1], di, dj)), (di, dj)
        assert np.array_equal(r["sum2"].astype(np.int64), shifted_sum(n_a, n_b, new[2], old[2], di, dj)), (di, dj)
        for p in range(7):
            want = shifted_sum(n_a, n_b, new[3][p * n:(p + 1) * n], old[3][p * n:(p + 1) * n], di, dj)
            assert np.array_equal(r["moments"][p * n:(p + 1) * n], want), (di, dj, sref.MOMENTS[p])


# ------------------------------------------------------------------------------------------------ 3. the point of the feature
def test_three_strips_are_fitted_by_the_window_alone():
    """tests/test_sectors_relief_cpu.py's example on the device: each strip alone is not fitted (by the slope session's own
    judgement of the same sums: a relief of depth 1), the window of three is, exactly; the terrain fed the same count, sum and
    sum2 calls the cell rough."""
    cfg = dict(JUDGE, n_a=2, n_b=2, window=0)
    h, alone = harness(3, **cfg), harness(1, **cfg)
    step = corner_step(0, 0)
    with d2pc.SectorsTerrain(h.cfg, depth=3) as terrain:
        t_out = {o: torch.zeros(4, dtype=torch.int32, device=DEV) for o in ("mean_q", "spread_q2")}
        t_flat = torch.zeros(4, dtype=torch.uint8, device=DEV)
        for u in (-5, 1, 7):
            frame = cases.sums_of(4, *cases.strip(u))
            a = alone.run(step, frame, what="strip %d alone" % u)
            assert not a["fitted"][0] and a["slope_a"][0] == a["slope_b"][0] == sref.NOT_FITTED and a["resid_q2"][0] == 84 and a["flat"][0] == 0
            r = h.run(step, frame, what="strip %d" % u)
            fc, fs, fs2, _ = frame_to_dev(frame)
            terrain.update(h.step, fc, fs, fs2, flat=t_flat, stream_ptr=stream(), **t_out)
        torch.cuda.synchronize()
        assert (int(t_out["mean_q"][0]), int(t_out["spread_q2"][0]), int(t_flat[0])) == (103, 300, 0), "the terrain: a spread of 300 > 200"
    assert r["status"].tolist() == [3, 3, 0, 0] and r["count"][0] == 24 and r["fitted"][0]
    assert sref.as_float(r["slope_a"])[0] == F32(0.1875) and sref.as_float(r["slope_b"])[0] == F32(0.125)
    assert r["resid_q2"][0] == 0 and r["level_q"][0] == 100 and r["flat"][0] == 1 and r["site"][0] == 1 and r["summary"].tolist() == [24, 1, 1, 1]
    h.reset()
    for u in (-5, 1, 7):
        r = h.run(step, cases.sums_of(4, *cases.strip(u, slope_u=5, slope_w=0)), what="steep strip %d" % u)
    assert r["fitted"][0] and sref.as_float(r["slope_a"])[0] == F32(0.3125) and r["resid_q2"][0] == 0 and r["flat"][0] == 0


# ------------------------------------------------------------------------------------------------ 4. the independent oracle
def test_three_clouds_through_slope_and_relief_equal_one_slope_call_over_all_three():
    """Real clouds, one step: slope_process_device then relief_update for each cloud; the window of the third update is, in
    all twelve outputs and bit for bit, what ONE slope call with n_clouds = 3 gives.  No reference code takes part."""
    Q = 1.0 / 512.0
    cfg = d2pc.sectors_ground_config_init(n_a=24, n_b=20, quantum=Q, min_count=4, max_step_q=20, window=1, w_dist=3, w_rough=1, max_spread_q2=60)
    scfg = d2pc.sectors_slope_config_init()
    n, k, cp, stride = 24 * 20, 7, 9000, 9100
    R64, t64, origin = gref.rotation(0.7, 0.25, -0.15), np.array([31.5, -47.25, 22.0]), np.array([28.0, -51.0, 21.0])
    rng = np.random.default_rng(26)
    a, b = rng.uniform(27.5, 40.5, 3 * stride), rng.uniform(-51.5, -40.5, 3 * stride)
    tilt = np.where(a > 36.0, 0.4 * (a - 36.0), 0.05 * (a - 28.0))                 # gentle ground, then a bank steeper than 15 degrees
    world = np.stack([a, b, origin[2] + 100 * Q + tilt + rng.normal(0.0, 3 * Q, 3 * stride)], axis=1)
    rough = b > -43.0
    world[rough, 2] += rng.normal(0.0, 14 * Q, int(rough.sum()))                    # a strip of rubble
    world[(a < 30.0) & (b < -49.0), 2] = np.nan                                     # and a hole: sixteen cells see nothing
    words = np.full((3 * stride, 4), 0x12345678, dtype=np.uint32)
    words[:, :3] = ((world - t64) @ R64).astype(F32).view(np.uint32)
    pts = to_dev(words, np.int32)
    step = to_dev(gref.step_words(R64, t64, origin, 11, 7), np.int32)
    with d2pc.SectorsSlope(cfg, scfg) as slope, d2pc.SectorsRelief(cfg, scfg, depth=3) as relief:
        want = fresh_outputs(n, k, SLOPE_OUT)
        slope.process(pts, cp, step, n_clouds=3, frame_stride_points=stride, n_candidates=k, stream_ptr=stream(), **want)
        frame = fresh_outputs(n, k, FRAME)
        for c in range(3):
            out = fresh_outputs(n, k)
            slope.process(pts[c * stride:], cp, step, stream_ptr=stream(), **frame)
            relief.update(step, frame["count"], frame["sum"], frame["sum2"], frame["moments"], n_candidates=k, stream_ptr=stream(), **out)
        torch.cuda.synchronize()
        want, got = read_outputs(want, n, k), read_outputs(out, n, k)
    assert got.pop("status").tolist() == [3, 3, 56, (-102) & OFF]
    for o in SLOPE_OUT:
        assert got[o].tobytes() == want[o].tobytes(), o
    points, n_flat, n_sites, n_fit = want["summary"].tolist()
    assert points > 15000 and 0 < n_sites < n_flat < n_fit < n and want["candidates"][k - 1] != NONE, want["summary"]
    assert want["candidates"][0] != want["candidates"][1]


# ------------------------------------------------------------------------------------------------ 5. the ring and h0
def test_ring_of_three_over_eight_updates_and_depth_one():
    h = harness(3, **dict(JUDGE, **GRIDS["5x3"]))
    rng = np.random.default_rng(8)
    frames = [cases.frame_tables(rng, 5, 3, 0, 0, fill=1.0) for _ in range(8)]
    for it, f in enumerate(frames):
        r = h.run(corner_step(0, 0), f, what="ring update %d" % it)
        assert r["status"].tolist() == [it + 1, min(it + 1, 3), 0, 0]
        window = frames[max(0, it - 2):it + 1]
        assert np.array_equal(r["count"], sum(w[0].astype(np.int64) for w in window)) and np.array_equal(r["moments"], sum(w[3] for w in window))
        hdr = h.read_state()[:256].view(np.uint32).reshape(16, 4)
        assert int(np.argmax(hdr[:3, 3])) == it % 3 and not hdr[3:].any(), "the smallest seq is replaced; headers beyond depth stay zero"
    one = harness(1, **dict(JUDGE, **GRIDS["5x3"]))
    for it, f in enumerate(frames[:3]):
        r = one.run(corner_step(it, 0), f, what="depth 1, update %d" % it)
        assert r["status"][:2].tolist() == [it + 1, 1]
        assert np.array_equal(r["count"], f[0]) and np.array_equal(r["sum"], f[1]) and np.array_equal(r["moments"], f[3]), "the frame alone"


def test_corners_round_half_to_even_and_anchor_up_to_2_to_the_29():
    h = harness(4, **dict(JUDGE, n_a=40, n_b=36, cell_size=1.0))
    rng = np.random.default_rng(22)
    for a0, b0, ia, jb in ((2.5, 3.5, 2, 4), (3.5, -0.5, 4, 0), (-0.5, -2.5, 0, -2), (-1.5, 0.49999997, -2, 0)):
        r = h.run(gref.step_words(cases.EYE, cases.ZERO, [a0, b0, 1.0]), cases.frame_tables(rng, 40, 36, ia, jb), what="corner (%r, %r)" % (a0, b0))
        assert r["status"][2:].tolist() == [ia & OFF, jb & OFF] and r["status"][1] == r["status"][0], "the four frames overlap"
    h.reset()
    top = 536870912.0
    below = float(np.nextafter(F32(top), F32(0)))               # 2^29 - 32: a neighbour 32 cells away
    assert top - below == 32.0
    frames = [cases.frame_tables(rng, 40, 36, 0, 0, fill=1.0) for _ in range(4)]
    r = h.run(gref.step_words(cases.EYE, cases.ZERO, [top, -top, 1.0]), frames[0], what="anchored at +-2^29")
    assert r["status"].tolist() == [1, 1, 1 << 29, (-(1 << 29)) & OFF]
    r = h.run(gref.step_words(cases.EYE, cases.ZERO, [below, -below, 1.0]), frames[1], what="the neighbour across")
    assert r["status"].tolist() == [2, 2, (1 << 29) - 32, (-(1 << 29) + 32) & OFF]
    assert np.array_equal(r["count"], shifted_sum(40, 36, frames[1][0], frames[0][0], -32, 32))
    r = h.run(gref.step_words(cases.EYE, cases.ZERO, [-top, top, 1.0]), frames[2], what="the opposite corner: a difference of 2^30")
    assert r["status"].tolist() == [3, 1, (-(1 << 29)) & OFF, 1 << 29]
    r = h.run(gref.step_words(cases.EYE, cases.ZERO, [-below, below, 1.0]), frames[3], what="its neighbour")
    assert r["status"][:2].tolist() == [4, 2]


def test_corners_beyond_the_anchor_nan_and_inf_leave_the_state_untouched():
    h = harness(3, **dict(JUDGE, **GRIDS["5x3"], cell_size=1.0))
    rng = np.random.default_rng(23)
    h.run(corner_step(0, 0, cell=1.0), cases.frame_tables(rng, 5, 3, 0, 0, fill=1.0), what="a first frame")
    h.run(corner_step(1, 0, cell=1.0), cases.frame_tables(rng, 5, 3, 1, 0, fill=1.0), what="a second frame")
    before = h.read_state()
    beyond = float(np.nextafter(F32(536870912.0), F32(np.inf)))
    for a0, b0 in ((beyond, 0.0), (0.0, -beyond), (np.nan, 0.0), (0.0, np.nan), (np.inf, 0.0), (0.0, -np.inf), (3e38, 3e38)):
        r = h.run(gref.step_words(cases.EYE, cases.ZERO, [a0, b0, 1.0], 2, 1), cases.frame_tables(rng, 5, 3, 0, 0, fill=1.0), k=3, what="corner (%r, %r)" % (a0, b0))
        assert np.array_equal(h.read_state(), before), "a frame that is not anchored wrote the state"
        assert r["status"].tolist() == [2, 0, 0, 0] and r["summary"].tolist() == [0, 0, 0, 0] and np.all(r["candidates"] == NONE)
        assert not r["count"].any() and not r["sum"].any() and not r["sum2"].any() and not r["moments"].any() and not r["flat"].any() and not r["site"].any()
        assert np.all(r["slope_a"] == 0x7FC00000) and np.all(r["slope_b"] == 0x7FC00000)
        assert np.all(r["level_q"] == -(1 << 31)) and np.all(r["resid_q2"] == 0xFFFFFFFF)
    r = h.run(corner_step(1, 1, cell=1.0), cases.frame_tables(rng, 5, 3, 1, 1, fill=1.0), what="anchored again")
    assert r["status"].tolist() == [3, 3, 1, 1]


def test_h0_drops_takes_up_again_signed_zeros_and_nan():
    h = harness(8, **dict(JUDGE, **GRIDS["5x3"]))
    rng = np.random.default_rng(24)
    took = []
    for h0 in (1.0, 1.0, 2.0, 1.0, 0.0, -0.0, np.nan, np.nan, -0.0, 1.0):
        r = h.run(corner_step(0, 0, h0=h0), cases.frame_tables(rng, 5, 3, 0, 0, fill=1.0), what="h0 %r" % h0)
        took.append(int(r["status"][1]))
    # 1.0 twice; 2.0 alone; back to 1.0: three; +0.0 alone; -0.0 equals it; NaN alone, twice; -0.0: three; the last 1.0 finds one other
    # 1.0 among the eight newest frames
    assert took == [1, 2, 1, 3, 1, 2, 1, 1, 3, 2]
    hdr = h.read_state()[:256].view(np.uint32).reshape(16, 4)
    assert sorted(hdr[:8, 2].tolist()).count(0x80000000) == 2 and (hdr[:8, 2] == 0x7FC00000).sum() == 2, "h0 is stored as its bits"


PER_CELL = ("count", "sum", "sum2", "moments", "slope_a", "slope_b", "level_q", "resid_q2", "flat", "status")


def test_counts_that_wrap_and_a_state_whose_seq_is_all_ones():
    h = harness(2, **dict(JUDGE, **GRIDS["2x2"]))
    pts = cases.sums_of(4, [1, 1, 1, 1], [10, 11, 9, 10], [-1, 1, 3, -3], [1, -1, 3, 5])
    big = (np.array([0x80000000, 4, 0, 0], dtype=np.uint32),) + pts[1:]
    h.run(corner_step(0, 0), big, what="2^31 points in a cell")
    r = h.run(corner_step(0, 0), big, what="and 2^31 more")
    assert r["count"].tolist() == [0, 8, 0, 0] and r["level_q"][0] == -(1 << 31) and r["resid_q2"][0] == 0xFFFFFFFF and r["slope_a"][0] == 0x7FC00000
    assert r["fitted"].tolist() == [False, True, False, False] and r["summary"][0] == 8
    # sums that wrap modulo 2^64 follow the formulas (the per-cell outputs are specified, site / candidates are not compared)
    mom = np.zeros(28, dtype=np.int64)
    mom[0::4] = [-(1 << 63), 1 << 62, -(1 << 63), 5, 1 << 62, -(1 << 63), 7]
    wrap = (np.array([1, 1, 1, 1], dtype=np.uint32), np.array([-(1 << 63), 5, 0, 0], dtype=np.int64), np.array([1 << 63, 25, 0, 0], dtype=np.uint64), mom)
    h.reset()
    h.run(corner_step(0, 0), wrap, want=PER_CELL, what="sums of 2^63")
    r = h.run(corner_step(0, 0), wrap, want=PER_CELL, what="wrapped sums")
    assert r["sum"][0] == 0 and r["sum2"][0] == 0 and r["count"][0] == 2 and r["moments"].reshape(7, 4)[:, 0].tolist() == [0, -(1 << 63), 0, 10, -(1 << 63), 0, 14]
    # a planted state: slot 1 holds seq 0xFFFFFFFF -> all slots are first taken as empty
    d3 = harness(3, **dict(JUDGE, **GRIDS["5x3"]))
    rng = np.random.default_rng(25)
    for it in range(3):
        d3.run(corner_step(it, 0), cases.frame_tables(rng, 5, 3, it, 0, fill=1.0), what="filling")
    state = d3.read_state()
    state[:256].view(np.uint32).reshape(16, 4)[1, 3] = 0xFFFFFFFF
    d3.plant_state(state)
    f = cases.frame_tables(rng, 5, 3, 1, 0, fill=1.0)
    r = d3.run(corner_step(1, 0), f, what="restart")
    assert r["status"].tolist() == [1, 1, 1, 0] and np.array_equal(r["count"], f[0])
    hdr = d3.read_state()[:256].view(np.uint32).reshape(16, 4)
    assert hdr[0].tolist() == [1, 0, F32(1.0).view(np.uint32), 1] and not hdr[1:].any(), "headers 1 .. depth - 1 are zeroed"
    r = d3.run(corner_step(1, 0), f, what="after the restart")
    assert r["status"].tolist() == [2, 2, 1, 0] and np.array_equal(r["count"], 2 * f[0]) and np.array_equal(r["moments"], 2 * f[3])
    # a planted seq of 0xFFFFFFFE steps to 0xFFFFFFFF, and the update after that restarts
    state = d3.read_state()
    state[:256].view(np.uint32).reshape(16, 4)[1, 3] = 0xFFFFFFFE
    d3.plant_state(state)
    assert d3.run(corner_step(1, 0), f, what="the last seq")["status"].tolist() == [0xFFFFFFFF, 3, 1, 0]
    assert d3.run(corner_step(1, 0), f, what="restart again")["status"].tolist() == [1, 1, 1, 0]


# ------------------------------------------------------------------------------------------------ 6. state and outputs
def test_save_restore_reset_and_two_runs_give_the_same_bytes():
    h = harness(4, **dict(JUDGE, n_a=16, n_b=16))
    rng = np.random.default_rng(27)
    frames = [cases.frame_tables(rng, 16, 16, i, -i) for i in range(5)]
    steps = [corner_step(i, -i, goal=(8, 8)) for i in range(5)]

    def sequence(first, last):
        return [h.device(steps[i], frames[i], k=6) for i in range(first, last)]

    def equal(a, b):
        return all(x[o].tobytes() == y[o].tobytes() for x, y in zip(a, b) for o in OUT)

    h.relief.reset(stream())
    run1 = sequence(0, 3)
    saved = h.state.clone()                                # one copy saves the map ...
    tail1 = sequence(3, 5)
    after = h.read_state()
    h.state.copy_(saved)                                   # ... and one restores it
    tail2 = sequence(3, 5)
    assert equal(tail1, tail2) and np.array_equal(h.read_state(), after), "restore, then the same two updates"
    assert tail1[1]["status"].tolist() == [5, 4, 4, (-4) & OFF]
    h.relief.reset(stream())
    hdr = h.read_state()[:256]
    assert not hdr.any() and np.array_equal(h.read_state()[256:], after[256:]), "reset zeroes the headers and nothing else"
    run2 = sequence(0, 3)
    assert equal(run1, run2) and run2[0]["status"].tolist() == [1, 1, 0, 0], "reset empties the window; two runs of one sequence"
    assert run2[2]["status"][1] == 3 and run2[2]["summary"][2] > 0 and run2[2]["summary"][3] > run2[2]["summary"][1]


def test_outputs_alone_and_together_and_refusals_enqueue_nothing():
    h = harness(3, **dict(JUDGE, n_a=16, n_b=16))
    rng = np.random.default_rng(28)
    allowed = (rng.random(256) < 0.9).astype(np.uint8)
    for it, want in enumerate([(o,) for o in OUT] + [("count", "summary"), ("flat", "site"), ("sum", "moments", "candidates", "status"), OUT]):
        ia, jb = it % 3, it % 2
        h.run(corner_step(ia, jb, goal=(7, 9)), cases.frame_tables(rng, 16, 16, ia, jb), allowed=allowed if it % 2 else None, k=7, want=want,
              what="outputs %s" % (want,))
    f = cases.frame_tables(rng, 16, 16, 1, 1)
    fc, fs, fs2, fm = frame_to_dev(f)
    out = fresh_outputs(h.n_cells, 5)
    lib = d2pc.load_sectors_library()
    before = h.read_state()
    state_ptr, state_bytes = h.relief.state()

    def status(check=True, **kw):
        args = dict(step=h.step.data_ptr(), frame_count=fc.data_ptr(), frame_sum=fs.data_ptr(), frame_sum2=fs2.data_ptr(), frame_moments=fm.data_ptr(),
                    n_candidates=5, **{o: t.data_ptr() for o, t in out.items()})
        desc = d2pc.sectors_relief_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_relief_update_device(h.relief.handle, ctypes.byref(desc), stream())
        assert st != 0 and (not check or st == d2pc.sectors_relief_desc_check(h.cfg, h.scfg, h.relief.tcfg, desc))
        return st

    assert status(struct_size=152) == 1 and "d2pc_sectors_relief_desc" in h.relief.last_error()
    assert status(step=None) == 1 and "step" in h.relief.last_error()
    assert status(frame_count=None) == 1 and status(frame_sum=None) == 1 and status(frame_sum2=None) == 1 and status(frame_moments=None) == 1
    assert "required" in h.relief.last_error()
    assert status(n_candidates=33) == 1 and "n_candidates" in h.relief.last_error()
    assert status(sum=out["sum"].data_ptr() + 4) == 1 and status(frame_moments=fm.data_ptr() + 4) == 1
    assert status(count=fc.data_ptr()) == 1 and "overlaps" in h.relief.last_error()
    assert status(moments=fm.data_ptr() + 8) == 1 and status(flat=out["site"].data_ptr() + 8) == 1
    assert status(**{o: None for o in OUT}) == 1
    # the session's own addition: its state block
    assert status(check=False, status=state_ptr + 16) == 1 and "state" in h.relief.last_error()
    assert status(check=False, summary=state_ptr + state_bytes - 16) == 1 and status(check=False, frame_moments=state_ptr + 256) == 1
    torch.cuda.synchronize()
    read_outputs(out, 0, 0)            # every entry still holds its sentinel
    assert np.array_equal(h.read_state(), before), "a refused update wrote the state"
    h.run(corner_step(1, 1), f, what="after the refusals")


# ------------------------------------------------------------------------------- 7. behind the producer and the slope, in a graph
def test_producer_slope_and_relief_in_one_captured_chain():
    """d2pc_process_device (COMPACT) -> d2pc_sectors_slope_process_device -> d2pc_sectors_relief_update_device captured once in
    one linear graph; two replays with new frames and a new 80-byte step copied into the same device words equal the eager
    result of the same chain and the reference.  An update that allocated, cleared with a memset node or read on the host
    would break the replays."""
    hh, w, border, f = 37, 70, 3, 2
    roi_n = (hh - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    k = 5
    judge = dict(min_count=4, max_spread_q2=d2pc.sectors_ground_spread_of_std(0.002, 0.8), max_step_q=400, window=1, w_dist=2)
    h = harness(4, max_slope=1.0, **judge)
    sh = sref.SectorsSlopeRef(h.cfg, h.scfg, d2pc.sectors_ground_geometry(h.cfg))
    nadir = np.array([[1.0, 0, 0], [0, -1.0, 0], [0, 0, -1.0]])        # the optical axis looks down
    poses = [(nadir, [0.0, 0.0, 10.0], [-4.0, -4.0, 8.0], 8, 8),
             (gref.rotation(0.3, 0.05, -0.04) @ nadir, [0.4, -0.2, 10.5], [-4.0, -4.5, 8.0], 3, 12),
             (gref.rotation(-1.1, -0.06, 0.02) @ nadir, [-0.3, 0.6, 9.5], [-4.5, -3.5, 8.0], OFF, 0)]
    d = torch.zeros((f, hh, w), dtype=torch.float32, device=DEV)
    pts = torch.full((f * stride, 4), 0x7FC5A5A5, dtype=torch.int32, device=DEV)
    counts = torch.zeros((f,), dtype=torch.int32, device=DEV)
    frame = fresh_outputs(h.n_cells, k, FRAME)
    out = fresh_outputs(h.n_cells, k)
    with d2pc.SectorsSlope(h.cfg, h.scfg) as slope, d2pc.Context(q=d2pc.make_q(fx=40.0, fy=40.0, cx=35.0, cy=18.0), border=border, compact_algo=1,
                                                                mode=d2pc.MODE_COMPACT) as ctx:
        def chain():
            s = stream()
            ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, hh, w * 4, hh * w * 4, f, pts.data_ptr(), None, stride,
                               counts.data_ptr(), s)
            slope.process(pts, roi_n, h.step, n_clouds=f, counts=counts, frame_stride_points=stride, stream_ptr=s, **frame)
            h.relief.update(h.step, frame["count"], frame["sum"], frame["sum2"], frame["moments"], n_candidates=k, stream_ptr=s, **out)

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
            part, cell, kq, u, wv = sh.bin(xyz, step)
            cells = sh.cells(cell[part], kq[part], u[part], wv[part])
            exp = h.ref.update(step, cells["count"], cells["sum"], cells["sum2"], cells["moments"], n_candidates=k)
            same(got, exp, what)
            assert np.array_equal(h.read_state(), h.ref.state), what
            return got

        ctx.reserve(w, hh, f)
        eager = {}
        for i in (0, 1, 2):
            feed(i)
            chain()
            torch.cuda.synchronize()
            eager[i] = check(i, "plain call %d" % i)
        assert eager[2]["status"][:2].tolist() == [3, 3] and eager[2]["summary"][0] > 2000 and eager[2]["summary"][3] > 0, "the window did not matter"
        before = h.ref.state.copy()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):              # (the capture is global: a device allocation inside it fails the call)
            chain()
        torch.cuda.synchronize()
        for i in (1, 2):                       # each replay against the eager run of the same chain from the same map
            h.plant_state(before)
            feed(i)
            chain()
            torch.cuda.synchronize()
            plain, plain_state = check(i, "eager step %d" % i), h.read_state()
            h.plant_state(before)
            feed(i)
            g.replay()
            torch.cuda.synchronize()
            replayed = check(i, "replay of step %d" % i)
            assert all(replayed[o].tobytes() == plain[o].tobytes() for o in OUT) and np.array_equal(h.read_state(), plain_state), i
            assert replayed["status"][:2].tolist() == [4, 4]
        ctx.check_async_error()
        del g
        ctx.release_graph_buffers()
