"""The elevation mode of include/d2pc_sectors.h (layer_kind = 1) restated in numpy float32, on top of
tests/sectors_ref.py: the sector, the key's reduction and the outputs are SectorsRef's; cells() is replaced.  One rounding
per operation (numpy's float32 ufuncs fuse nothing and np.sqrt on float32 is correctly rounded).  Both tables and the
geometry are ARGUMENTS, taken from the library (d2pc_sectors_table, d2pc_sectors_elevation_table,
d2pc_sectors_geometry)."""
import numpy as np

from sectors_ref import F32, SectorsRef


class SectorsElevRef(SectorsRef):
    def __init__(self, cfg, table, geometry, elevation_table):
        """elevation_table: (ce, se) float32, n_layers + 1 entries each."""
        super().__init__(cfg, table, geometry)
        assert int(cfg.layer_kind) == 1
        self.ce, self.se = (np.asarray(t, dtype=F32) for t in elevation_table)
        assert len(self.ce) == len(self.se) == self.layers + 1 == int(geometry.elevation_entries)

    def cells(self, xyz):
        """-> (takes_part bool, cell int64, d2 float32) of every point: the key is the Euclidean d2."""
        xyz = np.asarray(xyz, dtype=F32)
        f, l, u = self.flu(xyz)
        n = self.layers
        with np.errstate(all="ignore"):
            r2 = f * f + l * l
            h = np.sqrt(r2)
            d2 = r2 + u * u
            t = lambda i: self.ce[i] * u - self.se[i] * h  # noqa: E731
            part = np.isfinite(xyz[:, :3]).all(axis=1) & (r2 > 0) & (d2 >= self.rmin2) & (d2 <= self.rmax2)
            part &= (t(0) >= 0) & ~(t(n) >= 0)              # exactly so: a NaN t takes no part
            layer = np.zeros(len(xyz), dtype=np.int64)
            for i in range(1, n):
                layer += t(i) >= 0
            cross0 = self.c[0] * l - self.s[0] * f
            dot0 = self.c[0] * f + self.s[0] * l
            far = (cross0 < 0) | ((cross0 == 0) & (dot0 < 0))
            f, l = np.where(far, -f, f), np.where(far, -l, l)
            k = np.zeros(len(xyz), dtype=np.int64)
            for j in range(1, self.half):
                k += (self.c[j] * l - self.s[j] * f) >= 0
            assert h.dtype == d2.dtype == t(0).dtype == F32
        return part, layer * self.n + k + far * self.half, d2


def boundary_elevations(u_min, u_max, n_layers):
    """e_i in double, as the header forms them from the float32 band."""
    lo, hi = np.float64(F32(u_min)), np.float64(F32(u_max))
    return lo + (np.arange(n_layers + 1, dtype=np.float64) * (hi - lo)) / np.float64(n_layers)


def atan2_layer(f, l, u, u_min, u_max, n_layers):
    """float64 atan2 binning -> (inside the band bool, layer int64, distance to the nearest boundary in radians)."""
    e = boundary_elevations(u_min, u_max, n_layers)
    f, l, u = (np.asarray(v, dtype=np.float64) for v in (f, l, u))
    phi = np.arctan2(u, np.hypot(f, l))
    pos = (phi - e[0]) / ((e[-1] - e[0]) / n_layers)
    inside = (phi >= e[0]) & (phi < e[-1])
    layer = np.clip(np.floor(pos), 0, n_layers - 1).astype(np.int64)
    return inside, layer, np.abs(phi[:, None] - e[None, :]).min(axis=1)
