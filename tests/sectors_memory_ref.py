"""The memory of include/d2pc_sectors.h (d2pc_sectors_memory_*) restated in numpy float32, on top of tests/sectors_ref.py
and tests/sectors_elev_ref.py: a remembered point goes through the grid reference's own cells(), so the gate, the layer,
the sector and the key are SectorsRef's / SectorsElevRef's and the tables are the library's.  One rounding per operation
(numpy's float32 ufuncs fuse nothing); the carry key is min-reduced with np.minimum.at."""
import numpy as np

from sectors_ref import EMPTY_KEY, F32

EMPTY_AGE, OLDEST_AGE = 0xFFFFFFFF, 0xFFFFFFFE


def step_words(R, t, dt):
    """The 16 uint32 words of a d2pc_sectors_memory_step."""
    w = np.zeros(16, dtype=np.uint32)
    w[:9] = np.asarray(R, dtype=F32).reshape(9).view(np.uint32)
    w[9:12] = np.asarray(t, dtype=F32).reshape(3).view(np.uint32)
    w[12] = dt
    return w


class SectorsMemoryRef:
    def __init__(self, grid_ref, max_age):
        """grid_ref: the SectorsRef or SectorsElevRef of the grid's configuration."""
        self.ref, self.max_age = grid_ref, int(max_age)
        self.elevation = hasattr(grid_ref, "ce")
        self.n_cells = grid_ref.n_cells
        self.reset()

    def reset(self):
        self.records = np.zeros((self.n_cells, 4), dtype=np.uint32)
        self.records[:, 3] = EMPTY_AGE

    def to_points_frame(self, world, R, t):
        """Carry steps 2 and 3: R transposed on (w - t), one rounding per operation, summed left to right."""
        R, t = np.asarray(R, dtype=F32).reshape(9), np.asarray(t, dtype=F32).reshape(3)
        with np.errstate(all="ignore"):
            d = [world[:, i] - t[i] for i in range(3)]
            p = np.stack([(R[c] * d[0] + R[3 + c] * d[1]) + R[6 + c] * d[2] for c in range(3)], axis=1)
        assert p.dtype == F32
        return p

    def key_of(self, xyz):
        """k of a point: r2 from the picks for height layers, d2 for elevation layers."""
        f, l, u = self.ref.flu(xyz)
        with np.errstate(all="ignore"):
            k = f * f + l * l
            if self.elevation:
                k = k + u * u
        return k

    def carry(self, R, t, dt, covered=None):
        """-> (the cells' carry keys uint64, the aged age words uint32 of every old record)."""
        age = self.records[:, 3]
        aged = np.minimum(age.astype(np.uint64) + np.uint64(dt), np.uint64(OLDEST_AGE)).astype(np.uint32)
        kept = (age != EMPTY_AGE) & (aged <= self.max_age)
        p = self.to_points_frame(self.records[:, :3].copy().view(F32), R, t)
        part, cell, k = self.ref.cells(p)
        ok = kept & part
        if covered is not None:
            ok &= np.asarray(covered)[np.where(ok, cell, 0)] == 0
        key = (k.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.arange(self.n_cells, dtype=np.uint64)
        keys = np.full(self.n_cells, EMPTY_KEY, dtype=np.uint64)
        np.minimum.at(keys, cell[ok], key[ok])
        return keys, aged

    def update(self, words, count, nearest, bound, R, t, dt, covered=None):
        """One d2pc_sectors_memory_update_device.  words: the `points` buffer as uint32 (records, step words); count,
        nearest: what the sectors call wrote; bound: the call's position bound.
        -> dict(range float32, distance_cm uint16, age uint32, records uint32 (n_cells, 4)); the memory advances."""
        words = np.asarray(words).view(np.uint32)
        count, nearest = np.asarray(count).view(np.uint32), np.asarray(nearest).view(np.uint32)
        Rf, tf = np.asarray(R, dtype=F32).reshape(9), np.asarray(t, dtype=F32).reshape(3)
        keys, aged = self.carry(R, t, dt, covered)
        fresh = (count >= self.ref.min_count) & (nearest.astype(np.uint64) < np.uint64(bound))
        new = np.zeros((self.n_cells, 4), dtype=np.uint32)
        new[:, 3] = EMPTY_AGE
        rng = np.full(self.n_cells, np.inf, dtype=F32)
        with np.errstate(all="ignore"):
            q = words[nearest[fresh].astype(np.int64), :3].copy().view(F32)
            world = np.stack([((Rf[3 * r] * q[:, 0] + Rf[3 * r + 1] * q[:, 1]) + Rf[3 * r + 2] * q[:, 2]) + tf[r] for r in range(3)], axis=1)
            assert world.dtype == F32
            new[fresh, :3] = world.view(np.uint32)
            new[fresh, 3] = 0
            rng[fresh] = np.sqrt(self.key_of(q))
            kept = ~fresh & (keys != EMPTY_KEY)
            i = (keys[kept] & np.uint64(0xFFFFFFFF)).astype(np.int64)
            new[kept, :3] = self.records[i, :3]
            new[kept, 3] = aged[i]
            rng[kept] = np.sqrt((keys[kept] >> np.uint64(32)).astype(np.uint32).view(F32))
            seen = new[:, 3] != EMPTY_AGE
            cm = rng * F32(100.0)
            whole = np.where(seen & (cm < F32(65534.0)), cm, 0).astype(np.uint32)        # truncation towards zero
        cm = np.where(~seen, self.ref.no_obstacle_cm, np.where(cm >= F32(65534.0), 65534, whole)).astype(np.uint16)
        self.records = new
        return dict(range=rng, distance_cm=cm, age=new[:, 3].copy(), records=new.copy())


def rotation(yaw=0.0, pitch=0.0, roll=0.0, up=2):
    """A rotation matrix in double: `yaw` about axis `up` (0, 1, 2 = x, y, z), then pitch and roll about the other two."""
    def about(axis, a):
        m = np.eye(3)
        i, j = [(1, 2), (2, 0), (0, 1)][axis]
        m[i, i], m[i, j], m[j, i], m[j, j] = np.cos(a), -np.sin(a), np.sin(a), np.cos(a)
        return m
    return about(up, yaw) @ about((up + 1) % 3, pitch) @ about((up + 2) % 3, roll)
