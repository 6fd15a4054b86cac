"""The specification of include/d2pc_sectors.h restated in numpy float32: one rounding per operation (numpy's float32
ufuncs round every product, sum and square root once and fuse nothing), the cell's 64-bit key min-reduced with
np.minimum.at.  The boundary table and inv_h are ARGUMENTS: the tests hand over the library's own
(d2pc_sectors_table, d2pc_sectors_geometry), so a last-bit difference between two libms cannot move a bin."""
import numpy as np

EMPTY_KEY = np.uint64(0xFFFFFFFFFFFFFFFF)
F32 = np.float32


class SectorsRef:
    def __init__(self, cfg, table, geometry):
        """cfg: a SectorsConfig (or anything with its fields); table: (c, s) float32; geometry: rmin2, rmax2, inv_h."""
        self.n, self.layers = int(cfg.n_sectors), int(cfg.n_layers)
        self.half, self.n_cells = self.n // 2, self.n * self.layers
        self.axes = [int(a) for a in cfg.axes]
        self.c, self.s = (np.asarray(t, dtype=F32) for t in table)
        assert len(self.c) == len(self.s) == self.half
        self.rmin2, self.rmax2, self.inv_h = F32(geometry.rmin2), F32(geometry.rmax2), F32(geometry.inv_h)
        self.u_min, self.u_max = F32(cfg.u_min), F32(cfg.u_max)
        self.min_count, self.no_obstacle_cm = int(cfg.min_count), int(cfg.no_obstacle_cm)

    def flu(self, xyz):
        xyz = np.asarray(xyz, dtype=F32)
        return [(-xyz[:, abs(a) - 1] if a < 0 else xyz[:, abs(a) - 1]) for a in self.axes]   # a negation is exact

    def cells(self, xyz):
        """-> (takes_part bool, cell int64, r2 float32) of every point."""
        xyz = np.asarray(xyz, dtype=F32)
        f, l, u = self.flu(xyz)
        with np.errstate(all="ignore"):
            r2 = f * f + l * l
            part = np.isfinite(xyz[:, :3]).all(axis=1) & (r2 > 0) & (r2 >= self.rmin2) & (r2 <= self.rmax2)
            part &= (u >= self.u_min) & (u < self.u_max)
            layer = np.zeros(len(xyz), dtype=np.int64)
            if self.layers > 1:
                slab = np.floor((u - self.u_min) * self.inv_h)
                top = slab >= self.layers - 1
                layer = np.where(top, self.layers - 1, np.where(part & ~top, slab, 0)).astype(np.int64)
            cross0 = self.c[0] * l - self.s[0] * f
            dot0 = self.c[0] * f + self.s[0] * l
            far = (cross0 < 0) | ((cross0 == 0) & (dot0 < 0))
            f, l = np.where(far, -f, f), np.where(far, -l, l)
            k = np.zeros(len(xyz), dtype=np.int64)
            for j in range(1, self.half):
                k += (self.c[j] * l - self.s[j] * f) >= 0
        assert r2.dtype == F32 and cross0.dtype == F32
        return part, layer * self.n + k + far * self.half, r2

    def grid(self, xyz, positions):
        """-> dict(range float32, count uint32, nearest uint32, distance_cm uint16, keys uint64), n_cells entries each."""
        return self.reduce(*self.cells(xyz), positions)

    def reduce(self, part, cell, r2, positions):
        """grid() from what cells() gave (a test that reduces many prefixes of one cloud calls cells() once)."""
        key =(r2.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.asarray(positions).astype(np.uint64)
        keys = np.full(self.n_cells, EMPTY_KEY, dtype=np.uint64)
        np.minimum.at(keys, cell[part], key[part])
        count = np.bincount(cell[part], minlength=self.n_cells).astype(np.uint32)
        seen = count >= self.min_count
        r2_min = np.where(seen, (keys >> np.uint64(32)).astype(np.uint32), 0).astype(np.uint32).view(F32)
        with np.errstate(all="ignore"):
            rng = np.where(seen, np.sqrt(r2_min), F32(np.inf)).astype(F32)
            cm = rng * F32(100.0)
            whole = np.where(seen & (cm < F32(65534.0)), cm, 0).astype(np.uint32)        # truncation towards zero
        cm = np.where(~seen, self.no_obstacle_cm, np.where(cm >= F32(65534.0), 65534, whole)).astype(np.uint16)
        return dict(range=rng, count=count, nearest=(keys & np.uint64(0xFFFFFFFF)).astype(np.uint32), distance_cm=cm, keys=keys)


def gather(words, step_words, n_clouds, cloud_points, stride, counts=None):
    """The records a call visits: `words` is the `points` buffer as uint32 (records, step_words) -> (xyz float32,
    positions uint32), cloud after cloud; counts as the descriptor's (None, clamped, 0xFFFFFFFF = 0)."""
    words = np.asarray(words).view(np.uint32).reshape(-1, step_words)
    pos = []
    for c in range(n_clouds):
        n = cloud_points if counts is None else int(counts[c])
        n = 0 if n == 0xFFFFFFFF else min(n, cloud_points)
        pos.append(np.arange(n, dtype=np.int64) + c * (stride if n_clouds > 1 else 0))
    pos = np.concatenate(pos) if pos else np.zeros(0, dtype=np.int64)
    return words[pos, :3].copy().view(F32), pos.astype(np.uint32)


def atan2_sector(f, l, n_sectors, azimuth0):
    """float64 atan2 binning: what the count definition agrees with away from the boundaries."""
    a = np.mod(np.arctan2(np.asarray(l, dtype=np.float64), np.asarray(f, dtype=np.float64)) - azimuth0, 2 * np.pi)
    return np.minimum((a / (2 * np.pi / n_sectors)).astype(np.int64), n_sectors - 1)
