"""d2pc_sectors_memory_update_device on the GPU.  After EVERY call of a sequence range, distance_cm, age and records are
compared byte for byte with tests/sectors_memory_ref.py, which runs on the grid reference's own cells() with the library's
tables; every output is sentinel-filled with guard entries behind it.  The built cases seed the memory through a call
with a hand-made count / nearest (the kernel takes them as given), then assert the outcome itself beside the reference.
tests/README_sectors_memory.md has the map of cases."""
import ctypes

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import sectors_elev_ref
import sectors_memory_ref as mref
import sectors_ref
import test_sectors_elevation_gpu as elev
import test_sectors_gpu as base

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
F32 = np.float32
GUARD = 16
E = 0xFFFFFFFF
OUT = ("range", "distance_cm", "age", "records")
SENTINEL = dict(range=0x7FC3C3C3, distance_cm=0xA5C3, age=0x5A5AA5A5, records=0x3C3CC3C3)   # no call here produces them
DTYPE = dict(range=np.uint32, distance_cm=np.uint16, age=np.uint32, records=np.uint32)
SIGNED = dict(range=np.int32, distance_cm=np.int16, age=np.int32, records=np.int32)     # (torch has no unsigned 16 / 32)
WIDTH = dict(range=1, distance_cm=1, age=1, records=4)
HALF_PI = 1.5707964
EYE, ZERO = np.eye(3), np.zeros(3)

GRIDS = {
    "8x1": dict(n_sectors=8, r_min=0.3, r_max=30.0),                                          # the optical frame's axes
    "72x1": dict(axes=(1, 2, 3), r_min=0.2),
    "12x4": dict(n_sectors=12, n_layers=4, u_min=-4.0, u_max=6.0, axes=(1, 2, 3), r_min=0.5, r_max=25.0, azimuth0=0.3),
    "60x30e": dict(n_sectors=60, n_layers=30, layer_kind=1, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60, axes=(1, 2, 3),
                   r_min=0.3, r_max=40.0),                                                    # more cells than lanes
    "90x64e": dict(n_sectors=90, n_layers=64, layer_kind=1, u_min=-1.2, u_max=1.4, axes=(1, 2, 3), r_min=0.0),   # the largest table
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


def dev_words(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(DEV)


def grid_ref(cfg):
    table, geo = d2pc.sectors_table(cfg), d2pc.sectors_geometry(cfg)
    if cfg.layer_kind == d2pc.LAYERS_ELEVATION:
        return sectors_elev_ref.SectorsElevRef(cfg, table, geo, d2pc.sectors_elevation_table(cfg))
    return sectors_ref.SectorsRef(cfg, table, geo)


def fresh_outputs(n_cells, want=OUT):
    return {k: torch.from_numpy(np.full((n_cells + GUARD) * WIDTH[k], SENTINEL[k], dtype=DTYPE[k]).view(SIGNED[k])).to(DEV) for k in want}


def read_outputs(out, n_cells):
    """-> the outputs as numpy (bit patterns); asserts the guard entries behind each."""
    got = {}
    for k, t in out.items():
        a = t.cpu().numpy().view(DTYPE[k])
        assert np.all(a[n_cells * WIDTH[k]:] == SENTINEL[k]), "%s: an entry past n_cells was written" % k
        got[k] = a[:n_cells * WIDTH[k]].copy()
    return got


def same(got, want, what=""):
    for k, a in got.items():
        w = want[k].view(np.uint32).reshape(-1) if k in ("range", "records") else want[k].astype(DTYPE[k])
        bad = np.flatnonzero(a != w)
        assert bad.size == 0, "%s %s: entry %d is 0x%x, not 0x%x (%d differ)" % (what, k, bad[0], a[bad[0]], w[bad[0]], bad.size)


class Harness:
    """A sectors session, a memory session of its grid and the two references; update() runs one call of both and compares."""

    def __init__(self, max_age, **grid):
        self.sec = d2pc.Sectors(**grid)
        self.ref = grid_ref(self.sec.cfg)
        self.mem = d2pc.SectorsMemory(self.sec.cfg, max_age)
        self.mref = mref.SectorsMemoryRef(self.ref, max_age)
        self.n = self.sec.n_cells
        self.step = torch.zeros(16, dtype=torch.int32, device=DEV)

    def close(self):
        self.mem.close()
        self.sec.close()

    def reset(self):
        self.mem.reset(stream())
        self.mref.reset()

    def update(self, words, cloud_points, R=EYE, t=ZERO, dt=0, n_clouds=1, stride=0, step=16, counts=None, covered=None, want=OUT,
               seen=None, spare=0, what=""):
        """words: the `points` buffer as uint32 (records, step / 4).  seen: None runs d2pc_sectors_process_device for count
        and nearest; (count, nearest) hands them in as they are.  spare: records allocated behind `words`.
        -> the device's outputs, with 'grid' (the sectors reference's, when it ran) and 'sectors_range' (the device's)."""
        words = np.ascontiguousarray(words, dtype=np.uint32).reshape(-1, step // 4)
        pts = dev_words(np.concatenate([words, np.full((spare, step // 4), 0x7FC5A5A5, dtype=np.uint32)]))
        bound = (n_clouds - 1) * stride + cloud_points if n_clouds > 1 else cloud_points
        extra = {}
        if seen is None:
            s_out = dict(range=torch.zeros(self.n, dtype=torch.float32, device=DEV), count=torch.zeros(self.n, dtype=torch.int32, device=DEV),
                         nearest=torch.zeros(self.n, dtype=torch.int32, device=DEV))
            d_counts = dev_words(np.asarray(counts, dtype=np.uint32)) if counts is not None else None
            self.sec.process(pts, cloud_points, point_step=step, n_clouds=n_clouds, counts=d_counts, frame_stride_points=stride,
                             stream_ptr=stream(), **s_out)
            grid = self.ref.grid(*sectors_ref.gather(words, step // 4, n_clouds, cloud_points, stride, counts))
            count, nearest = grid["count"], grid["nearest"]
            d_count, d_nearest = s_out["count"], s_out["nearest"]
            extra = dict(grid=grid, sectors_out=s_out)
        else:
            count, nearest = (np.asarray(a, dtype=np.uint32) for a in seen)
            d_count, d_nearest = dev_words(count), dev_words(nearest)
        self.step.copy_(dev_words(d2pc.sectors_memory_step(R, t, dt)))
        d_cov = torch.from_numpy(np.asarray(covered, dtype=np.uint8)).to(DEV) if covered is not None else None
        out = fresh_outputs(self.n, want)
        self.mem.update(pts, cloud_points, d_count, d_nearest, self.step, point_step=step, n_clouds=n_clouds, frame_stride_points=stride,
                        covered=d_cov, stream_ptr=stream(), **out)
        torch.cuda.synchronize()
        got = read_outputs(out, self.n)
        exp = self.mref.update(words, count, nearest, bound, R, t, dt, covered)
        if seen is None:
            s = {k: v.cpu().numpy().view(np.uint32) for k, v in extra.pop("sectors_out").items()}
            assert np.array_equal(s["count"], count) and np.array_equal(s["nearest"], nearest), what + ": the sectors call itself"
            extra["sectors_range"] = s["range"]
        same(got, exp, what)
        return dict(exp, **extra)


def harness(name, max_age=1000, **over):
    """The harness of a grid, made once per module and emptied (d2pc_sectors_memory_reset_device) for every test."""
    key = (name, max_age, tuple(sorted(over.items())))
    if key not in _made:
        _made[key] = Harness(max_age, **dict(GRIDS[name], **over))
    _made[key].reset()
    return _made[key]


def records(xyz, step=16, seed=0):
    """xyz float32 (n, 3) -> uint32 records: the pad word and a textured record's second half are arbitrary bits."""
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 32, size=(len(xyz), step // 4), dtype=np.uint64).astype(np.uint32)
    w[:, :3] = np.ascontiguousarray(xyz, dtype=F32).view(np.uint32)
    return w


def from_flu(axes, f, l, u):
    """The xyz whose picks are f, l, u."""
    f, l, u = (np.atleast_1d(np.asarray(v, dtype=F32)) for v in (f, l, u))
    xyz = np.zeros((len(f), 3), dtype=F32)
    for a, v in zip(axes, (f, l, u)):
        xyz[:, abs(a) - 1] = -v if a < 0 else v
    return xyz


def wedge(axes, n, seed, fov=np.deg2rad(85.0), v_fov=np.deg2rad(60.0), far=20.0):
    """What one forward camera sees: n points inside a frustum about the forward axis, in the frame `axes` picks from."""
    rng = np.random.default_rng(seed)
    az, el = rng.uniform(-fov / 2, fov / 2, n), rng.uniform(-v_fov / 2, v_fov / 2, n)
    r = rng.uniform(0.4, far, n)
    return from_flu(axes, r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el))


def up_axis(axes):
    return abs(axes[2]) - 1


def yaw_pose(axes, yaw, pitch=0.0, roll=0.0):
    """A rotation about the frame's up axis (its sign makes a positive yaw turn from f towards l), with a little pitch and roll."""
    sign = -1.0 if axes[2] < 0 else 1.0
    return mref.rotation(sign * yaw, pitch, roll, up=up_axis(axes)).astype(F32)


def no_cloud(n):
    return np.zeros(n, dtype=np.uint32), np.full(n, E, dtype=np.uint32)


def seed_cells(h, points, cells, dt=0, R=EYE, t=ZERO, what="seed"):
    """Puts points[i] (in the frame of `points`) into the memory at cell cells[i], whatever cell it lies in: count 1 and
    nearest i there, nothing elsewhere."""
    count, nearest = no_cloud(h.n)
    count[cells], nearest[cells] = 1, np.arange(len(cells))
    return h.update(records(points), len(points), R, t, dt, seen=(count, nearest), what=what)


def xyz_at(r, c):
    """The record's world x, y, z of cell c, as float32."""
    return r["records"][c, :3].view(F32)


def is_point(a, p):
    return a.tobytes() == np.asarray(p, dtype=F32).tobytes()


def cell_of(h, xyz):
    part, cell, _ = h.ref.cells(np.asarray(xyz, dtype=F32).reshape(-1, 3))
    assert part.all()
    return cell


# ------------------------------------------------------------------------------------------------------- sequences
@pytest.mark.parametrize("name", list(GRIDS))
def test_sequence_identity_yaw_motion_and_an_empty_cloud(name):
    """Four calls of a vehicle that turns and moves: what left the field of view stays in the grid, ages, and goes at max_age."""
    h = harness(name, max_age=250)
    axes = list(h.sec.cfg.axes)
    cov = d2pc.sectors_memory_coverage(h.sec.cfg, [(0.0, 0.0, np.deg2rad(85.0), np.deg2rad(60.0), np.deg2rad(3.0))])
    assert 0 < cov.sum() < h.n
    climb = from_flu(axes, 0.0, 0.0, 0.8)[0]
    poses = [(EYE.astype(F32), ZERO, 0),
             (yaw_pose(axes, np.deg2rad(50.0)), ZERO, 100),
             (yaw_pose(axes, np.deg2rad(110.0), 0.03, -0.02), from_flu(axes, 1.5, -0.7, 0.0)[0] + climb, 100),
             (yaw_pose(axes, np.deg2rad(110.0), 0.03, -0.02), from_flu(axes, 1.5, -0.7, 0.0)[0] + climb, 100)]
    occupied = []
    for i, (R, t, dt) in enumerate(poses):
        n = 3000 + 17 * i
        words = records(wedge(axes, n, seed=100 + i))
        counts = [0] if i == 3 else None                   # the last call sees an empty cloud
        r = h.update(words, n, R, t, dt, counts=counts, covered=cov if i in (1, 2) else None, what="%s call %d" % (name, i))
        seen = r["grid"]["count"] >= h.ref.min_count
        occupied.append(r["age"] != E)
        assert np.all(r["age"][seen] == 0) and (seen.sum() >= 2 or i == 3)
        if i == 0:
            assert np.array_equal(occupied[0], seen)
            assert r["sectors_range"].tobytes() == r["range"].tobytes()
        if i in (1, 2):
            assert (occupied[i] & ~seen).sum() > 0, "nothing was remembered"
            assert not np.any(occupied[i] & ~seen & (cov != 0)), "a remembered point stayed where the cameras look"
    assert not r["grid"]["count"].any()
    ages = r["age"][occupied[3]]
    assert occupied[3].any() and set(ages.tolist()) <= {100, 200}, "call 0's records are 300 ticks old: beyond max_age"


def test_identity_pose_keeps_the_sectors_own_range_bits():
    """Identity pose, then an empty cloud: range is what d2pc_sectors_process_device wrote, bit for bit, and every age is dt."""
    for name in ("72x1", "12x4", "60x30e"):
        h = harness(name)
        xyz = (np.random.default_rng(5).normal(size=(4000, 3)) * 6.0).astype(F32)
        a = h.update(records(xyz), 4000, what=name + " first")
        assert a["sectors_range"].tobytes() == a["range"].tobytes() and (a["age"] == 0).sum() > 10
        b = h.update(records(xyz), 4000, dt=33, counts=[0], what=name + " second")
        assert b["range"].tobytes() == a["sectors_range"].tobytes()
        assert np.array_equal(b["age"], np.where(a["age"] == 0, 33, E)) and np.array_equal(b["records"][:, :3], a["records"][:, :3])


# ------------------------------------------------------------------------------------------------------ built cases
def test_two_remembered_points_in_one_cell_smaller_key_then_smaller_index():
    h = harness("72x1")
    near, far, twin = [3.0, 0.1, 0.5], [4.0, 0.1, -0.5], [3.0, 0.1, 7.0]       # one direction; twin has near's r2 and another z
    c = int(cell_of(h, [near])[0])
    assert c == cell_of(h, [far])[0] == cell_of(h, [twin])[0]
    seed_cells(h, [far, near], [9, 40])
    r = h.update(records(np.zeros((1, 3))), 1, dt=5, seen=no_cloud(h.n), what="smaller key")
    assert r["age"][c] == 5 and is_point(xyz_at(r, c), near) and (r["age"] != E).sum() == 1
    h.reset()
    seed_cells(h, [far, twin, near], [9, 50, 40])                # equal keys at records 40 and 50: the smaller index
    r = h.update(records(np.zeros((1, 3))), 1, dt=5, seen=no_cloud(h.n), what="smaller index")
    assert is_point(xyz_at(r, c), near)
    h.reset()
    seed_cells(h, [far, twin, near], [9, 40, 50])
    r = h.update(records(np.zeros((1, 3))), 1, dt=5, seen=no_cloud(h.n), what="smaller index, swapped")
    assert is_point(xyz_at(r, c), twin) and r["range"][c] == np.sqrt(F32(3.0) * F32(3.0) + F32(0.1) * F32(0.1))


def test_ages_max_age_saturation_and_dt_zero():
    h = harness("72x1", max_age=100)
    p = [[2.0, 1.0, 0.0]]
    c = int(cell_of(h, p)[0])
    seed_cells(h, p, [c])
    nothing = records(np.zeros((1, 3)))
    r = h.update(nothing, 1, dt=0, seen=no_cloud(h.n), what="dt 0")
    assert r["age"][c] == 0
    r = h.update(nothing, 1, dt=100, seen=no_cloud(h.n), what="a' == max_age")
    assert r["age"][c] == 100 and r["records"][c, :3].view(F32).tolist() == p[0]
    r = h.update(nothing, 1, dt=0, seen=no_cloud(h.n), what="dt 0 at max_age")
    assert r["age"][c] == 100
    r = h.update(nothing, 1, dt=1, seen=no_cloud(h.n), what="max_age + 1")
    assert np.all(r["age"] == E) and np.all(np.isinf(r["range"])) and not r["records"][:, :3].any()
    r = h.update(nothing, 1, dt=0xFFFFFFFF, seen=no_cloud(h.n), what="still empty")
    assert np.all(r["age"] == E)
    h = harness("72x1", max_age=0xFFFFFFFE)
    seed_cells(h, p, [c])
    r = h.update(nothing, 1, dt=0xFFFFFFFE, seen=no_cloud(h.n), what="exactly the oldest age")
    assert r["age"][c] == 0xFFFFFFFE
    r = h.update(nothing, 1, dt=0xFFFFFFFF, seen=no_cloud(h.n), what="saturated")
    assert r["age"][c] == 0xFFFFFFFE
    h.reset()
    seed_cells(h, p, [c])
    h.update(nothing, 1, dt=7, seen=no_cloud(h.n), what="7")
    r = h.update(nothing, 1, dt=0xFFFFFFFF, seen=no_cloud(h.n), what="7 + 0xFFFFFFFF does not wrap")
    assert r["age"][c] == 0xFFFFFFFE


def test_pushed_out_of_the_range_gate_and_the_height_slab():
    h = harness("12x4")                                  # r 0.5 .. 25, u -4 .. 6, body axes
    p = [[20.0, 0.0, 1.0], [0.2, 1.0, 1.0], [5.0, 5.0, 5.5], [5.0, -5.0, -3.5], [-6.0, 1.0, 0.0]]
    cells = np.arange(len(p))                            # (where a record lies in the buffer is of no matter)
    assert len(set(cell_of(h, p).tolist())) == len(p)
    nothing = records(np.zeros((1, 3)))
    moves = [([-6.0, 0.0, 0.0], [False, True, True, True, True]),        # backwards: the first is 26 away
             ([0.2, 0.8, 0.0], [True, False, True, True, True]),         # onto the second: 0.2 away, below r_min
             ([0.0, 0.0, -0.6], [True, True, False, True, True]),        # down: the third is 6.1 up
             ([0.0, 0.0, 0.6], [True, True, True, False, True])]         # up: the fourth is 4.1 down
    for t, stay in moves:
        h.reset()
        seed_cells(h, p, cells)
        r = h.update(nothing, 1, t=t, dt=1, seen=no_cloud(h.n), what="move %s" % t)
        left = {row[:3].tobytes() for row in r["records"] if row[3] != E}
        assert [np.asarray(q, dtype=F32).tobytes() in left for q in p] == stay, t


def test_pushed_out_of_the_elevation_band_and_the_euclidean_range():
    h = harness("60x30e", u_min=-0.5, u_max=0.6)         # r 0.3 .. 40 Euclidean
    p = [[10.0, 0.0, 6.0], [10.0, 1.0, -5.0], [30.0, 0.0, 20.0], [0.4, 0.0, 0.0]]
    cells = np.arange(len(p))
    assert len(set(cell_of(h, p).tolist())) == len(p)
    nothing = records(np.zeros((1, 3)))
    moves = [([0.0, 0.0, -1.5], [False, True, False, False]),     # down: atan(7.5 / 10) and atan(21.5 / 30) > 0.6; the fourth looks up
             ([0.0, 0.0, 1.0], [True, False, True, False]),       # up: atan(6 / 10.05) > 0.5 below; the fourth drops below the band
             ([0.2, 0.0, 0.0], [True, True, True, False]),        # forward: the fourth is 0.2 away, below r_min
             ([-9.0, 0.0, 0.0], [True, True, False, True])]       # backwards: the third is 43.8 away, inside the band
    for t, stay in moves:
        h.reset()
        seed_cells(h, p, cells)
        r = h.update(nothing, 1, t=t, dt=1, seen=no_cloud(h.n), what="move %s" % t)
        left = {row[:3].tobytes() for row in r["records"] if row[3] != E}
        assert [np.asarray(q, dtype=F32).tobytes() in left for q in p] == stay, t


def test_covered_drops_at_the_destination_cell_only():
    h = harness("72x1")
    p = [[4.0, 0.0, 0.0]]
    src = int(cell_of(h, p)[0])
    R = yaw_pose((1, 2, 3), np.deg2rad(40.0))            # the vehicle turns left: the point moves 8 sectors to the right
    dst = (src - 8) % 72
    nothing = records(np.zeros((1, 3)))
    for covered_cells, stays in (([src], True), ([dst], False), ([c for c in range(72) if c != dst], True)):
        h.reset()
        seed_cells(h, p, [src])
        cov = np.zeros(72, dtype=np.uint8)
        cov[covered_cells] = 200
        r = h.update(nothing, 1, R=R, dt=1, covered=cov, seen=no_cloud(h.n), what="covered %s" % covered_cells[:2])
        assert (r["age"][dst] == 1) == stays and (r["age"] != E).sum() == int(stays)


def test_a_cell_below_min_count_is_filled_from_the_memory():
    h = harness("72x1", min_count=2)
    pair = np.array([[5.0, 0.3, 0.0], [5.5, 0.3, 0.0]], dtype=F32)
    c = int(cell_of(h, pair[:1])[0])
    a = h.update(records(pair), 2, what="two points")
    assert a["grid"]["count"][c] == 2 and a["age"][c] == 0
    lone = np.array([[2.0, 0.1, 0.0]], dtype=F32)                    # nearer, in the same cell, but alone
    assert cell_of(h, lone)[0] == c
    b = h.update(records(lone), 1, dt=9, what="one point")
    assert b["grid"]["count"][c] == 1 and b["grid"]["nearest"][c] == 0 and np.isinf(b["sectors_range"].view(F32)[c])
    assert b["age"][c] == 9 and b["records"][c, :3].view(F32).tolist() == pair[0].tolist() and b["range"][c] == np.sqrt(F32(25.0) + F32(0.3) * F32(0.3))


@pytest.mark.parametrize("step", [16, 32])
def test_record_layouts_two_clouds_and_a_stride(step):
    h = harness("12x4")
    axes = (1, 2, 3)
    n, stride = 1500, 1511
    words = np.full((2 * stride, step // 4), 0x7FC5A5A5, dtype=np.uint32)      # NaN between the clouds
    words[:n] = records(wedge(axes, n, seed=31), step, seed=1)
    words[stride:stride + n] = records(wedge(axes, n, seed=32, fov=np.deg2rad(300.0)), step, seed=2)
    a = h.update(words[:stride + n], n, n_clouds=2, stride=stride, step=step, what="two clouds")
    assert (a["grid"]["nearest"][a["grid"]["count"] > 0] >= stride).any(), "no cell's nearest point is in the second cloud"
    R = yaw_pose(axes, np.deg2rad(-70.0), 0.02, 0.01)
    b = h.update(words[:n], n, R=R, t=[0.5, 0.25, -0.3], dt=40, step=step, what="one cloud, moved")
    assert ((b["age"] == 40).sum() > 3) and (b["age"] == 0).sum() > 3


def test_nearest_beyond_the_bound_counts_as_not_seen():
    """`points` is allocated a few records larger than the bound: whatever the kernel does with a `nearest` at or above
    the bound, no read leaves the buffer."""
    h = harness("72x1")
    p = np.array([[3.0, 0.0, 0.0], [0.0, 3.0, 0.0], [-3.0, 0.0, 0.0], [0.0, -3.0, 0.0]], dtype=F32)
    cells = cell_of(h, p)
    seed_cells(h, p[:1] * 2, cells[:1])                     # a remembered point behind the first cell
    count, nearest = no_cloud(h.n)
    count[cells] = 1
    nearest[cells] = [4, 1, 5, 3]                          # the bound is 4: positions 4 and 5 are not seen
    r = h.update(records(p), 4, dt=3, seen=(count, nearest), spare=8, what="beyond the bound")
    assert r["age"][cells].tolist() == [3, 0, E, 0] and r["records"][cells[0], :3].view(F32).tolist() == [6.0, 0.0, 0.0]
    nearest[cells] = [E, 0xFFFFFFFE, 1 << 31, 3]
    r = h.update(records(p), 4, dt=3, seen=(count, nearest), spare=8, what="far beyond the bound")
    assert r["age"][cells].tolist() == [6, 3, E, 0]
    # two clouds: the bound is stride + cloud_points
    words = np.concatenate([records(p), records(p * 2)])
    nearest[cells] = [0, 5, 7, 8]
    r = h.update(words, 3, n_clouds=2, stride=4, dt=1, seen=(count, nearest), spare=8, what="two clouds' bound")
    assert r["age"][cells].tolist() == [0, 0, E, 1] and r["records"][cells[1], :3].view(F32).tolist() == [0.0, 6.0, 0.0]


def test_outputs_alone_and_together():
    h = harness("12x4")
    axes = (1, 2, 3)
    subsets = [(k,) for k in OUT] + [("range", "age"), ("distance_cm", "records"), OUT]
    for i, want in enumerate(subsets):
        R = yaw_pose(axes, np.deg2rad(25.0 * i))
        h.update(records(wedge(axes, 900, seed=40 + i)), 900, R=R, t=[0.1 * i, 0.0, 0.05 * i], dt=20, want=want, what="outputs %s" % (want,))


def test_truncation_clamp_and_no_obstacle_cm():
    h = harness("8x1", r_max=np.inf, no_obstacle_cm=901)
    axes = list(h.sec.cfg.axes)
    f = np.array([0.305, 2.999, 655.34, 655.35, 3e6, 1e20], dtype=F32)
    ang = np.deg2rad(45.0) * np.arange(6) + 0.2
    p = from_flu(axes, f * np.cos(ang), f * np.sin(ang), np.zeros(6))
    cells = cell_of(h, p)
    assert len(set(cells.tolist())) == 6
    seed_cells(h, p, cells)
    r = h.update(records(np.zeros((1, 3))), 1, dt=1, seen=no_cloud(h.n), what="cm")
    cm = r["distance_cm"][cells].tolist()
    assert cm[0] == 30 and cm[1] == 299 and cm[4:] == [65534, 65534] and 65533 <= cm[2] <= 65534 and cm[3] == 65534
    assert np.all(r["distance_cm"][r["age"] == E] == 901)


def test_reset_and_same_bytes_again():
    h = harness("60x30e")
    axes = (1, 2, 3)
    runs = []
    for _ in range(2):
        h.reset()
        r = h.update(records(np.zeros((1, 3))), 1, dt=5, seen=no_cloud(h.n), what="after a reset")
        assert np.all(r["age"] == E) and np.all(np.isinf(r["range"]))
        a = h.update(records(wedge(axes, 2500, seed=51)), 2500, what="first")
        b = h.update(records(wedge(axes, 2500, seed=52)), 2500, R=yaw_pose(axes, 1.0), t=[0.3, 0.1, 0.2], dt=8, what="second")
        assert (b["age"] == 8).any()
        runs.append(a["records"].tobytes() + b["records"].tobytes() + b["range"].tobytes())
    assert runs[0] == runs[1]


def test_refusals_enqueue_nothing():
    h = harness("72x1")
    seed_cells(h, [[2.0, 0.5, 0.0]], [7])
    c = int(cell_of(h, [[2.0, 0.5, 0.0]])[0])
    words = records(wedge((1, 2, 3), 500, seed=97))
    pts = dev_words(words)
    count, nearest = (dev_words(a) for a in no_cloud(h.n))
    out = fresh_outputs(h.n)
    lib = d2pc.load_sectors_library()

    def status(**kw):
        args = dict(points=pts.data_ptr(), cloud_points=500, count=count.data_ptr(), nearest=nearest.data_ptr(), step=h.step.data_ptr(),
                    **{k: t.data_ptr() for k, t in out.items()})
        desc = d2pc.sectors_memory_desc_init(**dict(args, **kw))
        st = lib.d2pc_sectors_memory_update_device(h.mem.handle, ctypes.byref(desc), stream())
        assert st == d2pc.sectors_memory_desc_check(h.sec.cfg, h.mem.mcfg, desc)
        return st

    assert status(point_step=24) == 1 and "point_step" in h.mem.last_error()
    assert status(cloud_points=0) == 3 and status(range=pts.data_ptr() + 16) == 1 and "overlaps" in h.mem.last_error()
    assert status(age=out["range"].data_ptr() + 8) == 1 and status(n_clouds=2, points_frame_stride_points=499) == 3
    assert status(step=None) == 1 and status(nearest=None) == 1 and status(records=out["records"].data_ptr() + 8) == 1
    torch.cuda.synchronize()
    read_outputs(out, 0)           # every entry still holds its sentinel
    # and the memory did not advance: the next call ages the seeded record once
    r = h.update(words, 500, dt=4, seen=no_cloud(h.n), what="after the refusals")
    assert r["age"][c] == 4 and (r["age"] != E).sum() == 1


# ------------------------------------------------------------------------- the grid and the memory agree on the cell
RANGE_GATE = dict(axes=(1, 2, 3), r_min=0.5, r_max=25.0)   # rmin2 = 0.25, rmax2 = 625
AGREE = {
    "72x1": dict(n_sectors=72, **RANGE_GATE),
    "8x3": dict(n_sectors=8, n_layers=3, u_min=-0.7, u_max=1.9, azimuth0=0.3, **RANGE_GATE),
    "60x30e": dict(n_sectors=60, n_layers=30, layer_kind=1, u_min=-HALF_PI, u_max=HALF_PI, azimuth0=-np.pi / 60, **RANGE_GATE),
    "90x64e": dict(n_sectors=90, n_layers=64, layer_kind=1, u_min=-1.2, u_max=1.4, **RANGE_GATE),   # two carry passes
}
CARRY_PASS = 1024 * 3    # records of a carry pass: the block's lanes x the records a lane re-bins


def thinned(a, most):
    return a[::-(-len(a) // most)]


def agree_cloud(sec, ref):
    """Points on and next to the azimuth boundaries with l = +-0 and f < 0 among them, on the range gates' bit patterns, on
    the band's two boundaries and the layers' (elevation boundaries or slab edges), and a random cloud: the builders of
    tests/test_sectors_gpu.py and tests/test_sectors_elevation_gpu.py, thinned to a few thousand points."""
    axes, g = (1, 2, 3), sec.geometry
    elevation = sec.cfg.layer_kind == d2pc.LAYERS_ELEVATION
    xyz = [thinned(base.boundary_points(ref, axes), 1500)]
    lo, hi = elev.bits(g.rmin2), elev.bits(g.rmax2)
    for b in (lo - 1, lo, lo + 1, hi - 1, hi, hi + 1):
        fl = base.on_circle(b, seed=b & 0xFFFF)
        xyz.append(base.from_flu(axes, fl[:, 0], fl[:, 1], np.zeros(len(fl))))
        if elevation:
            xyz.append(elev.on_sphere(b, seed=b & 0xFFF))
    if elevation:
        xyz.append(thinned(elev.boundary_points(ref), 1500))
    else:
        edges = [F32(sec.cfg.u_min), F32(sec.cfg.u_max)] + [F32(F32(sec.cfg.u_min) + F32(k) / F32(g.inv_h)) for k in range(1, sec.cfg.n_layers)]
        us = np.array([v for e in edges if np.isfinite(e) for v in (np.nextafter(e, F32(-np.inf)), e, np.nextafter(e, F32(np.inf)))], dtype=F32)
        xyz.append(base.from_flu(axes, np.full(len(us), 2.0), np.linspace(-3, 3, len(us)), us))
    xyz.append(base.random_xyz(600, seed=77, spread=8.0))
    return np.concatenate(xyz).astype(F32)


@pytest.mark.parametrize("name", list(AGREE))
def test_a_remembered_point_lands_in_the_cell_the_grid_puts_it_in(name):
    """The two kernels against each other, not each against its own model.  A memory is seeded with a cloud's points (one
    per cell, as many cells at a time as the grid has), updated once more with no cloud, a pose, no `covered` and the
    largest max_age; the carried points R^T (w - t), formed on the host from the records the device stored with the
    reference's float arithmetic, go through an ordinary sectors call.  The cells that hold something and every range
    word of the two device results are the same bits.  Twice: under a yaw, pitch, roll and translation, and under the
    identity, where the carried points are the seeds themselves, on their boundaries."""
    sec = d2pc.Sectors(**AGREE[name])
    mem = d2pc.SectorsMemory(sec.cfg, d2pc.sectors.OLDEST_AGE)
    ref, n = grid_ref(sec.cfg), sec.n_cells
    model = mref.SectorsMemoryRef(ref, d2pc.sectors.OLDEST_AGE)
    cloud = agree_cloud(sec, ref)
    assert 500 < len(cloud) <= 4500
    part = ref.cells(cloud)[0]
    assert part.sum() > 100 and (~part).sum() > 100, "the cloud lies on both sides of the gates"
    step = torch.zeros(16, dtype=torch.int32, device=DEV)
    poses = [(yaw_pose((1, 2, 3), 0.6458, 0.03, -0.02), np.array([0.4, -0.1, 0.9]), 7), (EYE, ZERO, 1)]
    held = second_pass = 0
    for R, t, dt in poses:
        for first in range(0, len(cloud), n):
            batch = cloud[first:first + n]
            m = len(batch)
            cells = np.arange(m) * n // m           # spread over the whole table: records of both carry passes
            count, nearest = no_cloud(n)
            count[cells], nearest[cells] = 1, np.arange(m)
            pts = dev_words(records(batch, seed=first))
            mem.reset(stream())
            step.copy_(dev_words(d2pc.sectors_memory_step(EYE, ZERO, 0)))
            seeded = fresh_outputs(n, ("records",))
            mem.update(pts, m, dev_words(count), dev_words(nearest), step, stream_ptr=stream(), **seeded)
            torch.cuda.synchronize()
            rec = read_outputs(seeded, n)["records"].reshape(n, 4)
            assert np.array_equal(np.flatnonzero(rec[:, 3] != E), cells), "the seeds are in the memory"
            # the update under test: nothing seen, everything carried
            step.copy_(dev_words(d2pc.sectors_memory_step(R, t, dt)))
            out = fresh_outputs(n, ("range", "age"))
            mem.update(pts, m, dev_words(no_cloud(n)[0]), dev_words(no_cloud(n)[1]), step, stream_ptr=stream(), **out)
            torch.cuda.synchronize()
            got = read_outputs(out, n)
            # the carried points, as records of a cloud of their own, through the grid's kernel
            carried = model.to_points_frame(rec[cells, :3].copy().view(F32), R, t)
            grid = base.run(sec, dev_words(records(carried, seed=first + 1)), m, want=("range", "count"))
            what = "%s, points %d.., dt %d" % (name, first, dt)
            assert np.array_equal(got["age"] != E, grid["count"] > 0), what + ": the cells that hold something"
            bad = np.flatnonzero(got["range"] != grid["range"])
            assert bad.size == 0, "%s: range of cell %d is 0x%x from the memory, 0x%x from the grid (%d differ)" % (
                what, bad[0], got["range"][bad[0]], grid["range"][bad[0]], bad.size)
            assert np.all(got["age"][got["age"] != E] == dt)
            held += int((got["age"] != E).sum())
            second_pass += int(ref.cells(carried)[0][cells >= CARRY_PASS].sum())
    assert held > 100, "the memory held nothing to compare"
    assert (second_pass > 0) == (n > CARRY_PASS), "the second carry pass took part exactly where the table needs it"
    mem.close()
    sec.close()


# ------------------------------------------------------------------------------------- behind the producer, in a graph
PT_SENTINEL = 0x7FC5A5A5


def disparities(f, h, w, seed, holes=0.3):
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 64.0, size=(f, h, w)).astype(F32)
    d[rng.random(size=d.shape) < holes] = 0.0
    return d


def test_producer_sectors_and_memory_in_one_captured_chain():
    """d2pc_process_device (COMPACT) -> d2pc_sectors_process_device -> d2pc_sectors_memory_update_device captured once; three
    replays with new input and `step` rewritten between them equal three plain calls of a second memory session, and the
    reference.  A call that allocated, or a parity kept on the host, would break the replays."""
    hh, w, border, f = 37, 70, 3, 2
    roi_n = (hh - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    h = harness("12x4", n_sectors=36, axes=(3, -1, -2), u_min=-3.0, u_max=3.0, r_min=0.05)
    axes = (3, -1, -2)
    plain = d2pc.SectorsMemory(h.sec.cfg, 1000)
    d = torch.zeros((f, hh, w), dtype=torch.float32, device=DEV)
    pts = torch.full((f * stride, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros((f,), dtype=torch.int32, device=DEV)
    s_out = dict(count=torch.zeros(h.n, dtype=torch.int32, device=DEV), nearest=torch.zeros(h.n, dtype=torch.int32, device=DEV))
    out = fresh_outputs(h.n)
    steps = [(yaw_pose(axes, 0.0), np.zeros(3), 0), (yaw_pose(axes, 1.1, 0.02, 0.01), np.array([0.05, -0.02, 0.1]), 30),
             (yaw_pose(axes, 2.3, -0.01, 0.03), np.array([-0.1, 0.03, 0.2]), 45)]
    with d2pc.Context(q=d2pc.make_q(fx=40.0, fy=40.0, cx=35.0, cy=18.0), border=border, compact_algo=1, mode=d2pc.MODE_COMPACT) as ctx:
        def chain(memory):
            s = stream()
            ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, hh, w * 4, hh * w * 4, f, pts.data_ptr(), None, stride,
                               counts.data_ptr(), s)
            h.sec.process(pts, roi_n, n_clouds=f, counts=counts, frame_stride_points=stride, stream_ptr=s, **s_out)
            memory.update(pts, roi_n, s_out["count"], s_out["nearest"], h.step, n_clouds=f, frame_stride_points=stride,
                          stream_ptr=s, **out)

        def feed(i):
            d.copy_(torch.from_numpy(disparities(f, hh, w, 70 + i)))
            h.step.copy_(dev_words(d2pc.sectors_memory_step(*steps[i])))

        ctx.reserve(w, hh, f)
        want = []
        for i in range(3):
            feed(i)
            chain(plain)
            torch.cuda.synchronize()
            got = read_outputs(out, h.n)
            words = pts.cpu().numpy().view(np.uint32).reshape(-1, 4)
            cn = counts.cpu().numpy().view(np.uint32)
            grid = h.ref.grid(*sectors_ref.gather(words, 4, f, roi_n, stride, cn))
            same(got, h.mref.update(words, grid["count"], grid["nearest"], stride * (f - 1) + roi_n, *steps[i]), "plain call %d" % i)
            want.append(got)
        assert np.isin(want[2]["age"], (45, 75)).any() and (want[2]["age"] == 0).any(), "the memory did not matter"
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            chain(h.mem)
        torch.cuda.synchronize()
        for i in range(3):
            feed(i)
            g.replay()
            torch.cuda.synchronize()
            got = read_outputs(out, h.n)
            for k in OUT:
                assert got[k].tobytes() == want[i][k].tobytes(), "replay %d: %s differs from the plain call" % (i, k)
        ctx.check_async_error()
        del g
        ctx.release_graph_buffers()
    plain.close()
