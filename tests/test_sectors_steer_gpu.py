"""d2pc_sectors_steer_device on the GPU.  Every call's clearance_cm, cost, candidates and summary are compared byte for byte
with tests/sectors_steer_ref.py (the direct 2-D window of the specification, on the library's reach tables); every output is
sentinel-filled with guard entries behind it.  The built cases assert the outcome itself beside the reference.
tests/README_sectors_steer.md has the map of cases."""
import ctypes

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_ref
import sectors_steer_ref as sref
import test_sectors_memory_gpu as mem

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
GUARD = 16
NOTHING, BLOCKED, OFF = 65535, 0xFFFFFFFF, 0xFFFFFFFF
NONE = 0xFFFFFFFFFFFFFFFF
OUT = ("clearance_cm", "cost", "candidates", "summary")
SENTINEL = dict(clearance_cm=0xA5C3, cost=0x5A5AA5A5, candidates=0x3C3CC3C35A5AA5A5, summary=0x7FC3C3C3)   # no call here produces them
DTYPE = dict(clearance_cm=np.uint16, cost=np.uint32, candidates=np.uint64, summary=np.uint32)
SIGNED = dict(clearance_cm=np.int16, cost=np.int32, candidates=np.int64, summary=np.int32)     # (torch has no unsigned 16 / 32 / 64)
HALF_PI = 1.5707964

# grid, steer configuration.  8x1: Wa = n / 2; 60x30e: more cells than lanes; 90x64e: 5,760 cells, every lane's several
# cells; its tables are the largest a test here uses
GRIDS = {
    "8x1": (dict(n_sectors=8), dict(radius=0.5, max_reach_sectors=4, max_reach_layers=0)),
    "72x1": (dict(), dict(radius=0.5, max_reach_sectors=8, max_reach_layers=0)),
    "12x4": (dict(n_sectors=12, n_layers=4, u_min=-2.0, u_max=2.0), dict(radius=0.75, max_reach_sectors=3, max_reach_layers=2)),
    "8x3": (dict(n_sectors=8, n_layers=3, u_min=-1.5, u_max=1.5), dict(radius=0.75, max_reach_sectors=3, max_reach_layers=2)),
    "60x30e": (dict(n_sectors=60, n_layers=30, layer_kind=1, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60),
               dict(radius=0.5, max_reach_sectors=8, max_reach_layers=4)),
    "90x64e": (dict(n_sectors=90, n_layers=64, layer_kind=1, u_min=-1.2, u_max=1.2), dict(radius=1.0, max_reach_sectors=16, max_reach_layers=8)),
}
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
    size = dict(clearance_cm=n_cells, cost=n_cells, candidates=k, summary=4)
    return {o: to_dev(np.full(size[o] + GUARD, SENTINEL[o], dtype=DTYPE[o]), SIGNED[o]) for o in want}


def read_outputs(out, n_cells, k):
    """-> the outputs as numpy; asserts the guard entries behind each."""
    size = dict(clearance_cm=n_cells, cost=n_cells, candidates=k, summary=4)
    got = {}
    for o, t in out.items():
        a = t.cpu().numpy().view(DTYPE[o])
        assert np.all(a[size[o]:] == SENTINEL[o]), "%s: an entry past its end was written" % o
        got[o] = a[:size[o]].copy()
    return got


def same(got, want, what=""):
    for o, a in got.items():
        w = want[o].astype(DTYPE[o])
        bad = np.flatnonzero(a != w)
        assert bad.size == 0, "%s %s: entry %d is 0x%x, not 0x%x (%d differ)" % (what, o, bad[0], a[bad[0]], w[bad[0]], bad.size)


class Harness:
    """A steer session and its reference (on the library's reach tables); run() makes one call of both and compares."""

    def __init__(self, grid, steer):
        self.cfg = d2pc.sectors_config_init(**grid)
        self.scfg = d2pc.sectors_steer_config_init(**steer)
        self.steer = d2pc.SectorsSteer(self.cfg, self.scfg)
        self.reach_s, self.reach_l = d2pc.sectors_steer_reach(self.cfg, self.scfg)
        self.ref = sref.SectorsSteerRef(self.cfg, self.scfg, self.reach_s, self.reach_l)
        self.n, self.layers, self.n_cells = self.cfg.n_sectors, self.cfg.n_layers, self.steer.n_cells
        self.step = torch.zeros(8, dtype=torch.int32, device=DEV)

    def close(self):
        self.steer.close()

    def empty(self, fill=NOTHING):
        return np.full(self.n_cells, fill, dtype=np.uint16)

    def cell(self, s, l=0):
        return l * self.n + s % self.n

    def device(self, d, step, allowed, k, want):
        """One d2pc_sectors_steer_device -> the outputs as numpy."""
        self.step.copy_(to_dev(step, np.int32))
        d_dev = to_dev(np.asarray(d, dtype=np.uint16), np.int16)
        a_dev = torch.from_numpy(np.asarray(allowed, dtype=np.uint8)).to(DEV) if allowed is not None else None
        out = fresh_outputs(self.n_cells, k, want)
        self.steer.steer(d_dev, self.step, allowed=a_dev, n_candidates=k, stream_ptr=stream(), **out)
        torch.cuda.synchronize()
        return read_outputs(out, self.n_cells, k)

    def run(self, d, step=None, allowed=None, k=5, want=OUT, what=""):
        """-> the reference's result, which the device's equals bit for bit."""
        step = sref.step_words() if step is None else np.asarray(step, dtype=np.uint32)
        got = self.device(d, step, allowed, k, want)
        exp = self.ref.steer(d, step, allowed, k)
        same(got, exp, what)
        return exp


def harness(name, grid=None, **steer):
    """The harness of a grid and a steer configuration, made once per module."""
    key = (name, tuple(sorted((grid or {}).items())), tuple(sorted(steer.items())))
    if key not in _made:
        _made[key] = Harness(dict(GRIDS[name][0], **(grid or {})), dict(GRIDS[name][1], **steer))
    return _made[key]


def key_of(cost, cell):
    return (int(cost) << 32) | int(cell)


# ------------------------------------------------------------------------------------------------ the reach, entry by entry
@pytest.mark.parametrize("name", list(GRIDS))
def test_one_obstacle_at_every_reach_entry(name):
    """One obstacle at reach, reach + 1 and reach - 1 cm for every k of both tables; in elevation mode in the lowest, a middle
    and the highest layer (the row of reach_s is the SOURCE's layer).  The cell k sectors (layers) away is widened into
    exactly when the obstacle is within that entry."""
    h = harness(name)
    elevation = h.cfg.layer_kind == d2pc.LAYERS_ELEVATION
    rows = sorted({0, h.layers // 2, h.layers - 1}) if elevation else [h.layers // 2]
    s0 = 5 % h.n
    calls = 0
    for l in rows:
        for k in range(1, h.ref.wa + 1):
            reach = int(h.reach_s[l, k])
            for v in (reach - 1, reach, reach + 1):
                d = h.empty()
                d[h.cell(s0, l)] = v
                r = h.run(d, want=("clearance_cm", "summary"), what="%s layer %d k %d v %d" % (name, l, k, v))
                calls += 1
                clr = r["clearance_cm"].reshape(h.layers, h.n)
                within = v <= reach and v < NOTHING
                for side in (s0 + k, s0 - k):
                    assert clr[l, side % h.n] == (v if within else NOTHING), (l, k, v, side)
                assert clr[l, s0] == v and r["summary"][1] == min(v, NOTHING)
                nearer = [j for j in range(1, k) if v <= h.reach_s[l, j]]     # (the tables are monotone: within k means within every j < k)
                assert not within or len(nearer) == k - 1
    for k in range(1, h.ref.we + 1):
        reach = int(h.reach_l[k])
        for l in sorted({0, h.layers // 2, h.layers - 1}):
            for v in (reach - 1, reach, reach + 1):
                if v < 0:
                    continue
                d = h.empty()
                d[h.cell(s0, l)] = v
                r = h.run(d, want=("clearance_cm",), what="%s layers: layer %d k %d v %d" % (name, l, k, v))
                calls += 1
                clr = r["clearance_cm"].reshape(h.layers, h.n)
                within = v <= reach and v < NOTHING
                for j in (l + k, l - k):
                    if 0 <= j < h.layers:
                        assert clr[j, s0] == (v if within else NOTHING), (l, k, v, j)
    assert calls >= 3 * (h.ref.wa + h.ref.we)


def test_height_layers_reach_one_slab_and_none():
    """Slabs of 1.0 against a radius of 0.75: half a slab away is within the vehicle (any range), one and a half is not
    (the entry is 0: an obstacle at 0 cm alone passes it)."""
    for name in ("12x4", "8x3"):
        h = harness(name)
        assert h.reach_l.tolist() == [65535, 65534, 0]
        for v, two_away in ((65534, NOTHING), (300, NOTHING), (1, NOTHING), (0, 0)):
            d = h.empty()
            d[h.cell(2, 0)] = v
            clr = h.run(d, what="%s v %d" % (name, v))["clearance_cm"].reshape(h.layers, h.n)
            assert clr[0, 2] == v and clr[1, 2] == v and clr[2, 2] == two_away
            assert np.all(clr[3:] == NOTHING)


# ------------------------------------------------------------------------------------------------ the seam and the poles
def test_the_seam_and_the_far_cell_reached_from_both_sides():
    h = harness("72x1")
    v = int(h.reach_s[0, 3])                                   # within three sectors, not within four
    assert v > h.reach_s[0, 4]
    for s0 in (0, 71):
        d = h.empty()
        d[s0] = v
        clr = h.run(d, what="seam, sector %d" % s0)["clearance_cm"]
        want = h.empty()
        want[[(s0 + j) % 72 for j in range(-3, 4)]] = v
        assert np.array_equal(clr, want)
    d = h.empty()
    assert h.reach_s[0, 2] < 400 and h.reach_s[0, 1] >= 500
    d[0], d[71] = 500, 400                                     # both within one sector, neither within two
    clr = h.run(d, what="both sides of the seam")["clearance_cm"]
    assert clr[[70, 71, 0, 1]].tolist() == [400, 400, 400, 500] and clr[2] == NOTHING and clr[69] == NOTHING
    # Wa = n / 2 on the 8-sector grid: the cell opposite is reached with ks = +4 and ks = -4, the same cell
    h = harness("8x1")
    assert h.ref.wa == 4 and h.reach_s[0].tolist() == [65535, 130, 54, 50, 50]   # 2.5 and 3.5 x 45 degrees are beyond pi / 2: floor(100 rho)
    for v, beyond in ((50, 50), (51, NOTHING)):
        d = h.empty()
        d[6] = v
        clr = h.run(d, what="opposite, v %d" % v)["clearance_cm"]
        assert clr[2] == beyond and np.all(clr[[1, 3]] == beyond) and np.all(clr[[4, 5, 6, 7, 0]] == v)


@pytest.mark.parametrize("name", ["12x4", "8x3", "60x30e", "90x64e"])
def test_layers_do_not_wrap(name):
    """An obstacle in layer 0 (L - 1) that every reach entry lets through lowers the We layers above (below) it and no other:
    nothing wraps over the pole or below the lowest slab."""
    h = harness(name)
    for l0 in (0, h.layers - 1):
        d = h.empty()
        d[h.cell(3, l0)] = 0
        clr = h.run(d, what="%s layer %d" % (name, l0))["clearance_cm"].reshape(h.layers, h.n)
        touched = np.flatnonzero((clr != NOTHING).any(axis=1))
        reach = max([k for k in range(h.ref.we + 1) if h.reach_l[k] >= 0])
        want = np.arange(0, reach + 1) if l0 == 0 else np.arange(h.layers - 1 - reach, h.layers)
        assert np.array_equal(touched, want), (l0, touched)


# ------------------------------------------------------------------------------------------------ the separable form
def test_two_obstacles_in_one_row_against_the_direct_window():
    """Row 15 of the 60 x 30 grid, target cell one layer up.  The obstacle straight below the target is too far away to be
    widened upwards (it fails reach_l[1]); the one two sectors aside is near enough for reach_l[1] and passes or fails the
    row's reach_s[2].  The azimuth pass's minimum must not let one obstacle's verdict stand for the other's."""
    h = harness("60x30e")
    rl1, rs2 = int(h.reach_l[1]), int(h.reach_s[15, 2])
    assert rs2 < rl1 < 2000 and h.reach_s[15, 1] >= rl1 - 1
    for aside, above in ((rs2, rs2), (rs2 + 1, NOTHING), (rs2 - 1, rs2 - 1)):
        d = h.empty()
        d[h.cell(20, 15)], d[h.cell(22, 15)] = 2000, aside
        clr = h.run(d, what="aside %d" % aside)["clearance_cm"].reshape(30, 60)
        assert clr[16, 20] == above and clr[14, 20] == above, aside
        assert clr[15, 20] == (aside if aside <= rs2 else 2000) and clr[16, 22] == aside and clr[15, 22] == aside
    # the nearer obstacle straight below passes reach_l[1]: it wins whatever the farther one does
    d = h.empty()
    d[h.cell(20, 15)], d[h.cell(22, 15)] = rl1, rs2 + 1
    clr = h.run(d, what="below passes")["clearance_cm"].reshape(30, 60)
    assert clr[16, 20] == rl1 and clr[16, 22] == rs2 + 1 and clr[16, 21] == rs2 + 1


# ------------------------------------------------------------------------------------------------ the input's mapping
def test_free_cm_mapping():
    h = harness("72x1", free_cm=2001)
    d = h.empty(2001)                                   # a grid whose no_obstacle_cm is 2001
    d[[10, 30, 50, 60]] = [0, 2000, 2001, 65535]
    r = h.run(d, what="free_cm 2001")
    clr = r["clearance_cm"]
    assert clr[10] == 0 and clr[30] == 2000 and clr[50] == NOTHING and clr[60] == NOTHING and r["summary"][1] == 0
    assert (clr == 2000).sum() == 1 and (clr == 0).sum() == 17, "2000 cm is beyond every neighbour's reach; 0 cm is within all 8"
    d = h.empty(2001)
    r = h.run(d, what="nothing but no_obstacle_cm")
    assert np.all(r["clearance_cm"] == NOTHING) and r["summary"].tolist() == [72, NOTHING, 0, 0]
    h = harness("72x1")                                 # free_cm 65535: 65534 is an obstacle, far beyond reach
    d = h.empty()
    d[7] = 65534
    r = h.run(d, what="65534")
    assert r["clearance_cm"][7] == 65534 and (r["clearance_cm"] != NOTHING).sum() == 1 and r["summary"][1] == 65534
    h = harness("72x1", free_cm=0)                      # everything is nothing
    r = h.run(np.arange(72, dtype=np.uint16), what="free_cm 0")
    assert np.all(r["clearance_cm"] == NOTHING) and r["summary"].tolist() == [72, NOTHING, 0, 0]


# ------------------------------------------------------------------------------------------------ free
def test_min_clearance_and_allowed():
    h = harness("72x1", min_clearance_cm=300, max_reach_sectors=0)
    d = h.empty()
    d[[4, 5, 6]] = [299, 300, 301]
    r = h.run(d, what="min_clearance_cm")
    assert r["cost"][4] == BLOCKED and r["cost"][5] != BLOCKED and r["cost"][6] != BLOCKED and r["summary"][0] == 71
    r = h.run(d, allowed=np.zeros(72, dtype=np.uint8), what="nothing allowed")
    assert np.all(r["cost"] == BLOCKED) and r["summary"][0] == 0 and np.all(r["candidates"] == NONE)
    r = h.run(d, allowed=np.full(72, 200, dtype=np.uint8), what="everything allowed, by any nonzero byte")
    assert r["summary"][0] == 71
    wedge = d2pc.sectors_memory_coverage(h.cfg, [(0.0, 0.0, np.deg2rad(87.0), np.deg2rad(58.0), np.deg2rad(2.0))])
    assert 0 < wedge.sum() < 72 and wedge[0] == 1 and wedge[36] == 0
    r = h.run(d, allowed=wedge, k=32, what="a forward wedge")
    free = np.flatnonzero(r["cost"] != BLOCKED)
    assert np.array_equal(free, np.flatnonzero((wedge != 0) & (np.arange(72) != 4))) and r["summary"][0] == len(free)
    h = harness("60x30e", min_clearance_cm=0)            # 0: a cell on an obstacle at 0 cm is free all the same
    d = h.empty()
    d[100] = 0
    r = h.run(d, what="min_clearance_cm 0")
    assert r["summary"][0] == 1800 and r["cost"][100] != BLOCKED


# ------------------------------------------------------------------------------------------------ the cost
def test_cost_terms_switched_off_and_clamped():
    h = harness("12x4", w_near=0)
    n, layers = 12, 4
    d = h.empty()
    s, l = np.meshgrid(np.arange(n), np.arange(layers))
    ring = lambda a: np.minimum(np.abs(s - a), n - np.abs(s - a))  # noqa: E731
    for step, want in (((OFF, 0, OFF, 0), 0 * s),
                       ((n, 1, 0xFFFFFFFE, 2), 0 * s),                                     # n and 0xFFFFFFFE are off as well
                       ((3, 1, OFF, 0), 16 * (ring(3) + np.abs(l - 1))),
                       ((OFF, 0, 7, 2), 4 * (ring(7) + np.abs(l - 2))),
                       ((3, 1, 7, 2), 16 * (ring(3) + np.abs(l - 1)) + 4 * (ring(7) + np.abs(l - 2))),
                       ((3, layers, 7, 0xFFFFFFFF), 16 * (ring(3) + np.abs(l - 3)) + 4 * (ring(7) + np.abs(l - 3))),   # clamped to L - 1
                       ((0, 0, 11, 3), 16 * (ring(0) + l) + 4 * (ring(11) + np.abs(l - 3)))):   # across the seam, both directions
        r = h.run(d, step=sref.step_words(*step), k=5, what="step %s" % (step,))
        assert np.array_equal(r["cost"], want.reshape(-1).astype(np.uint32)), step
        if not want.any():
            assert r["candidates"].tolist() == [key_of(0, c) for c in range(5)], "everything free at one cost: cells 0 .. K - 1"
    r = h.run(d, step=sref.step_words(0, 0, 11, 3), what="the seam")
    assert r["cost"][11] == 16 * 1 + 4 * 3 and r["cost"][h.cell(0, 3)] == 16 * 3 + 4 * 1 and r["cost"][h.cell(6, 0)] == 16 * 6 + 4 * (5 + 3)


def test_largest_cost_and_horizon():
    grid = dict(n_sectors=360, n_layers=16, u_min=0.0, u_max=16.0)
    h = harness("72x1", grid=grid, w_goal=4095, w_prev=4095, w_near=4095, horizon_cm=65535, min_clearance_cm=0, max_reach_sectors=0)
    d = h.empty()
    far = h.cell(180, 15)
    d[far] = 0                                          # clearance 0, half a turn and 15 layers from the goal and the previous heading
    r = h.run(d, step=sref.step_words(0, 0, 0, 0), k=1, what="the largest cost")
    assert r["cost"][far] == 4095 * (65535 + 2 * (180 + 15)) == r["cost"].max() and r["cost"][far] < BLOCKED
    assert r["candidates"][0] == key_of(0, 0) and r["summary"].tolist() == [5760, 0, 0, 0]
    h = harness("72x1", horizon_cm=0, w_goal=0, w_prev=0, w_near=4095, min_clearance_cm=0)
    d = h.empty()
    d[[3, 40]] = [0, 500]
    r = h.run(d, what="horizon_cm 0")
    assert not r["cost"].any(), "nothing is nearer than a horizon of 0"
    h = harness("72x1", horizon_cm=1000, w_goal=0, w_prev=0, w_near=3, min_clearance_cm=0, max_reach_sectors=0)
    d[[3, 40, 41, 42]] = [0, 999, 1000, 1001]
    r = h.run(d, what="horizon_cm 1000")
    assert r["cost"][[3, 40, 41, 42, 50]].tolist() == [3000, 3, 0, 0, 0]


# ------------------------------------------------------------------------------------------------ the candidates
@pytest.mark.parametrize("k", [1, 5, 32])
def test_candidates_ascending_ties_by_cell(k):
    h = harness("60x30e", w_prev=0, w_near=0, min_clearance_cm=0)
    d = h.empty()
    goal = (17, 11)
    r = h.run(d, step=sref.step_words(*goal), k=k, what="K %d" % k)
    s, l = np.meshgrid(np.arange(60), np.arange(30))
    dist = (np.minimum(np.abs(s - 17), 60 - np.abs(s - 17)) + np.abs(l - 11)).reshape(-1)
    order = np.lexsort((np.arange(1800), dist))[:k]       # by distance, then by cell
    assert r["candidates"].tolist() == [key_of(16 * dist[c], c) for c in order]
    assert r["candidates"][0] == key_of(0, h.cell(*goal))
    if k >= 5:
        assert [int(c) & 0xFFFFFFFF for c in r["candidates"][1:5]] == [h.cell(17, 10), h.cell(16, 11), h.cell(18, 11), h.cell(17, 12)]


def test_fewer_free_cells_than_candidates_and_none():
    h = harness("72x1", w_near=0, min_clearance_cm=0)
    d = h.empty()
    allowed = np.zeros(72, dtype=np.uint8)
    allowed[[70, 3, 40]] = 1
    r = h.run(d, step=sref.step_words(2, 0), allowed=allowed, k=32, what="three free cells")
    assert r["candidates"][:3].tolist() == [key_of(16, 3), key_of(16 * 4, 70), key_of(16 * 34, 40)]
    assert np.all(r["candidates"][3:] == NONE) and r["summary"][0] == 3
    r = h.run(d, allowed=np.zeros(72, dtype=np.uint8), k=32, what="no free cell")
    assert np.all(r["candidates"] == NONE) and r["summary"].tolist() == [0, NOTHING, 0, 0]
    r = h.run(d, allowed=allowed, k=3, what="exactly K free cells")
    assert r["candidates"].tolist() == [key_of(0, 3), key_of(0, 40), key_of(0, 70)]
    h = harness("72x1", min_clearance_cm=100)
    r = h.run(h.empty(0), k=5, what="an obstacle everywhere")
    assert np.all(r["candidates"] == NONE) and r["summary"].tolist() == [0, 0, 0, 0]


def test_candidates_over_the_whole_block():
    """5,760 cells: all free at one cost; the winner in the last cell; the winner in cells the last lane of the last wave
    holds (1,023 and 5,119: lane 1,023 takes the cells 1,023 + 1,024 j)."""
    h = harness("90x64e", w_prev=0, w_near=0, min_clearance_cm=0)
    d = h.empty()
    r = h.run(d, k=32, what="one cost")
    assert r["candidates"].tolist() == [key_of(0, c) for c in range(32)] and r["summary"][0] == 5760
    for cell in (5759, 1023, 5119, 1024, 63, 64):
        s, l = cell % 90, cell // 90
        r = h.run(d, step=sref.step_words(s, l), k=5, what="the winner in cell %d" % cell)
        assert r["candidates"][0] == key_of(0, cell) and (int(r["candidates"][1]) >> 32) == 16
    only = np.zeros(5760, dtype=np.uint8)
    only[[5759, 5119]] = 1
    r = h.run(d, allowed=only, k=5, what="two free cells at the block's end")
    assert r["candidates"].tolist() == [key_of(0, 5119), key_of(0, 5759), NONE, NONE, NONE]
    # a random grid: every lane's cells differ in cost
    rng = np.random.default_rng(8)
    d = np.where(rng.random(5760) < 0.08, rng.integers(0, 3000, 5760), NOTHING).astype(np.uint16)
    h = harness("90x64e", min_clearance_cm=150)
    r = h.run(d, step=sref.step_words(44, 30, 50, 33), allowed=(rng.random(5760) < 0.9).astype(np.uint8), k=32, what="a random grid")
    assert 0 < r["summary"][0] < 5760 and np.all(np.diff(r["candidates"].astype(np.float64)) > 0) and (r["clearance_cm"] < d).any()


def test_one_lane_holds_every_winner_in_a_row():
    """The only free cells are 7, 1,031, 2,055 and 3,079: lane 7 of the block holds all four, in its slots 0 .. 3, so the
    same lane wins round after round and looks for its next key each time.  Without a goal every cost is equal and the
    candidates come in slot order; with the goal on the last of them the lane's best key sits in its last slot."""
    h = harness("90x64e", w_prev=0, w_near=0, min_clearance_cm=0)
    d = h.empty()
    cells = [7, 1031, 2055, 3079]
    only = np.zeros(5760, dtype=np.uint8)
    only[cells] = 1
    r = h.run(d, allowed=only, k=5, what="four free cells of one lane, one cost")
    assert r["candidates"].tolist() == [key_of(0, c) for c in cells] + [NONE] and r["summary"][0] == 4
    r = h.run(d, step=sref.step_words(3079 % 90, 3079 // 90), allowed=only, k=5, what="four free cells of one lane, the goal on the last")
    assert r["candidates"][0] == key_of(0, 3079) and r["candidates"][4] == NONE
    assert sorted(int(c) & 0xFFFFFFFF for c in r["candidates"][:4]) == cells and np.all(np.diff(r["candidates"][:4].astype(np.float64)) > 0)


@pytest.mark.parametrize("name", list(GRIDS))
def test_random_grids(name):
    h = harness(name)
    rng = np.random.default_rng(h.n_cells)
    for i, occupancy in enumerate((0.02, 0.08, 0.5, 1.0)):
        entries = np.unique(np.concatenate([h.reach_s.reshape(-1), h.reach_l]).astype(np.int64))
        pool = np.clip(np.concatenate([entries - 1, entries, entries + 1]), 0, 65535)
        v = np.where(rng.random(h.n_cells) < 0.5, pool[rng.integers(0, len(pool), h.n_cells)], rng.integers(0, 3000, h.n_cells))
        d = np.where(rng.random(h.n_cells) < occupancy, v, NOTHING).astype(np.uint16)
        step = sref.step_words(int(rng.integers(0, h.n)), int(rng.integers(0, h.layers)), int(rng.integers(0, h.n)), int(rng.integers(0, h.layers)))
        allowed = (rng.random(h.n_cells) < 0.8).astype(np.uint8) if i % 2 else None
        r = h.run(d, step=step, allowed=allowed, k=(1, 5, 32, 7)[i], what="%s occupancy %g" % (name, occupancy))
        if occupancy <= 0.08 and h.n_cells >= 1000:
            assert (r["clearance_cm"] < h.ref.mapped(d).reshape(-1)).any(), "no obstacle was widened"


# ------------------------------------------------------------------------------------------------ the outputs
def test_outputs_alone_in_pairs_and_together_and_the_same_bytes_again():
    h = harness("60x30e")
    rng = np.random.default_rng(3)
    d = np.where(rng.random(1800) < 0.1, rng.integers(0, 2500, 1800), NOTHING).astype(np.uint16)
    step = sref.step_words(10, 12, 14, 15)
    subsets = [(o,) for o in OUT] + [(a, b) for i, a in enumerate(OUT) for b in OUT[i + 1:]] + [OUT]
    for want in subsets:
        h.run(d, step=step, k=5, want=want, what="outputs %s" % (want,))
    first = h.device(d, step, None, 32, OUT)
    again = h.device(d, step, None, 32, OUT)
    for o in OUT:
        assert first[o].tobytes() == again[o].tobytes(), o


def test_refusals_return_desc_checks_status_and_enqueue_nothing():
    h = harness("72x1")
    d = to_dev(h.empty(), np.int16)
    out = fresh_outputs(72, 5)
    lib = d2pc.load_sectors_library()

    def status(**kw):
        args = dict(distance_cm=d.data_ptr(), step=h.step.data_ptr(), n_candidates=5, **{o: t.data_ptr() for o, t in out.items()})
        desc = d2pc.sectors_steer_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_steer_device(h.steer.handle, ctypes.byref(desc), stream())
        assert st == d2pc.sectors_steer_desc_check(h.cfg, h.scfg, desc) and st != 0
        return st

    assert status(struct_size=60) == 1 and "d2pc_sectors_steer_desc" in h.steer.last_error()
    assert status(distance_cm=None) == 1 and status(step=None) == 1 and "step" in h.steer.last_error()
    assert status(n_candidates=0) == 1 and status(n_candidates=33) == 1 and "n_candidates" in h.steer.last_error()
    assert status(cost=out["cost"].data_ptr() + 2) == 1 and status(candidates=out["candidates"].data_ptr() + 4) == 1
    assert status(summary=d.data_ptr() + 140) == 1 and "overlaps" in h.steer.last_error()
    assert status(clearance_cm=out["cost"].data_ptr() + 8) == 1 and status(cost=h.step.data_ptr()) == 1
    assert status(clearance_cm=None, cost=None, candidates=None, summary=None) == 1
    torch.cuda.synchronize()
    read_outputs(out, 0, 0)            # every entry still holds its sentinel
    h.run(h.empty(), what="after the refusals")


# ------------------------------------------------------------------------------------- behind the producer, in a graph
def test_producer_sectors_memory_and_steer_in_one_captured_chain():
    """d2pc_process_device (COMPACT) -> d2pc_sectors_process_device -> d2pc_sectors_memory_update_device ->
    d2pc_sectors_steer_device captured once; three replays with new frames and both steps rewritten between them equal three
    plain calls of a second set of sessions, and those equal the references.  A call that allocated, or a goal kept on the
    host, would break the replays."""
    hh, w, border, f = 37, 70, 3, 2
    roi_n = (hh - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    axes = (3, -1, -2)
    m = mem.Harness(1000, **dict(mem.GRIDS["12x4"], n_sectors=36, axes=axes, u_min=-3.0, u_max=3.0, r_min=0.05))
    steer_kw = dict(radius=1.0, max_reach_sectors=4, max_reach_layers=1, min_clearance_cm=60, horizon_cm=800)
    scfg = d2pc.sectors_steer_config_init(**steer_kw)
    captured, plain_steer = d2pc.SectorsSteer(m.sec.cfg, scfg), d2pc.SectorsSteer(m.sec.cfg, scfg)
    plain_mem = d2pc.SectorsMemory(m.sec.cfg, 1000)
    ref = sref.SectorsSteerRef(m.sec.cfg, scfg, *d2pc.sectors_steer_reach(m.sec.cfg, scfg))
    assert ref.reach_l.tolist() == [65535, 65534]
    k = 5
    d = torch.zeros((f, hh, w), dtype=torch.float32, device=DEV)
    pts = torch.full((f * stride, 4), mem.PT_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros((f,), dtype=torch.int32, device=DEV)
    s_out = dict(count=torch.zeros(m.n, dtype=torch.int32, device=DEV), nearest=torch.zeros(m.n, dtype=torch.int32, device=DEV))
    m_out = mem.fresh_outputs(m.n, ("distance_cm", "age"))
    out = fresh_outputs(m.n, k)
    goal = torch.zeros(8, dtype=torch.int32, device=DEV)
    poses = [(mem.yaw_pose(axes, 0.0), np.zeros(3), 0), (mem.yaw_pose(axes, 1.1, 0.02, 0.01), np.array([0.05, -0.02, 0.1]), 30),
             (mem.yaw_pose(axes, 2.3, -0.01, 0.03), np.array([-0.1, 0.03, 0.2]), 45)]
    goals = [sref.step_words(0, 1, OFF, 0), sref.step_words(30, 2, 0, 1), sref.step_words(17, 3, 30, 2)]
    with d2pc.Context(q=d2pc.make_q(fx=40.0, fy=40.0, cx=35.0, cy=18.0), border=border, compact_algo=1, mode=d2pc.MODE_COMPACT) as ctx:
        def chain(memory, steer):
            s = stream()
            ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, hh, w * 4, hh * w * 4, f, pts.data_ptr(), None, stride,
                               counts.data_ptr(), s)
            m.sec.process(pts, roi_n, n_clouds=f, counts=counts, frame_stride_points=stride, stream_ptr=s, **s_out)
            memory.update(pts, roi_n, s_out["count"], s_out["nearest"], m.step, n_clouds=f, frame_stride_points=stride, stream_ptr=s, **m_out)
            steer.steer(m_out["distance_cm"], goal, n_candidates=k, stream_ptr=s, **out)

        def feed(i):
            d.copy_(torch.from_numpy(mem.disparities(f, hh, w, 70 + i)))
            m.step.copy_(mem.dev_words(d2pc.sectors_memory_step(*poses[i])))
            goal.copy_(to_dev(goals[i], np.int32))

        ctx.reserve(w, hh, f)
        want = []
        for i in range(3):
            feed(i)
            chain(plain_mem, plain_steer)
            torch.cuda.synchronize()
            got = read_outputs(out, m.n, k)
            words = pts.cpu().numpy().view(np.uint32).reshape(-1, 4)
            cn = counts.cpu().numpy().view(np.uint32)
            grid = m.ref.grid(*sectors_ref.gather(words, 4, f, roi_n, stride, cn))
            remembered = m.mref.update(words, grid["count"], grid["nearest"], stride * (f - 1) + roi_n, *poses[i])
            mem.same(mem.read_outputs(m_out, m.n), remembered, "plain call %d, the memory" % i)
            same(got, ref.steer(remembered["distance_cm"], goals[i], None, k), "plain call %d" % i)
            want.append(got)
        assert 0 < want[2]["summary"][0] < m.n and (want[2]["clearance_cm"] < remembered["distance_cm"]).any(), "the steer did not matter"
        assert want[1]["candidates"].tobytes() != want[2]["candidates"].tobytes()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            chain(m.mem, captured)
        torch.cuda.synchronize()
        for i in range(3):
            feed(i)
            g.replay()
            torch.cuda.synchronize()
            got = read_outputs(out, m.n, k)
            for o in OUT:
                assert got[o].tobytes() == want[i][o].tobytes(), "replay %d: %s differs from the plain call" % (i, o)
        ctx.check_async_error()
        del g
        ctx.release_graph_buffers()
    for s in (captured, plain_steer, plain_mem, m):
        s.close()
