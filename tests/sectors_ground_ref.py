"""The GROUND block of include/d2pc_sectors.h restated in numpy: float32 with an explicit astype after every operation for
the binning (one rounding per operation, nothing fused), Python / int64 integers for the moments.  S is computed DIRECTLY as
the sum of (k - m)^2, not by the wrapped formula the kernel uses: the two forms check each other.  inv_c and inv_q are
ARGUMENTS: the tests hand over the library's own (d2pc_sectors_ground_geometry)."""
import numpy as np

F32 = np.float32
EMPTY_MEAN, EMPTY_SPREAD = 0x80000000, 0xFFFFFFFF
NO_CANDIDATE = 0xFFFFFFFFFFFFFFFF
MAX_K = 32767


def step_words(R, t, origin, goal_i=0xFFFFFFFF, goal_j=0xFFFFFFFF):
    """The 20 words of a d2pc_sectors_ground_step as uint32."""
    w = np.zeros(20, dtype=np.uint32)
    w[:9] = np.asarray(R, dtype=F32).reshape(9).view(np.uint32)
    w[9:12] = np.asarray(t, dtype=F32).reshape(3).view(np.uint32)
    w[12:15] = np.asarray(origin, dtype=F32).reshape(3).view(np.uint32)
    w[15], w[16] = goal_i, goal_j
    return w


def rotation(yaw, pitch, roll):
    """Rz(yaw) Ry(pitch) Rx(roll) in float64."""
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    rz = np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]])
    ry = np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
    rx = np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]])
    return rz @ ry @ rx


def wrapped_spread_sum(count, total, total2, m):
    """S by the kernel's formula, sum2 - 2 m sum + count m^2, every operation modulo 2^64 (Python integers)."""
    mask = (1 << 64) - 1
    um, us = m & mask, total & mask
    return (total2 - ((2 * um) & mask) * us + (count * um & mask) * um) & mask


class SectorsGroundRef:
    def __init__(self, cfg, geometry):
        """cfg: a SectorsGroundConfig (or anything with its fields); geometry: inv_c, inv_q."""
        self.n_a, self.n_b = int(cfg.n_a), int(cfg.n_b)
        self.n_cells = self.n_a * self.n_b
        self.axes = [int(a) for a in cfg.axes]
        self.inv_c, self.inv_q = F32(geometry.inv_c), F32(geometry.inv_q)
        self.min_count, self.max_spread_q2, self.max_step_q = int(cfg.min_count), int(cfg.max_spread_q2), int(cfg.max_step_q)
        self.window, self.w_dist, self.w_rough, self.rough_cap = int(cfg.window), int(cfg.w_dist), int(cfg.w_rough), int(cfg.rough_cap)

    # ---------------------------------------------------------------------------------------------------- per record
    def world(self, xyz, step):
        """Steps 1 and 2 -> (finite bool, w float32 (n, 3))."""
        xyz = np.asarray(xyz, dtype=F32).reshape(-1, 3)
        s = np.asarray(step, dtype=np.uint32)
        R, t = s[:9].view(F32), s[9:12].view(F32)
        x, y, z = xyz[:, 0], xyz[:, 1], xyz[:, 2]
        w = np.zeros((len(xyz), 3), dtype=F32)
        with np.errstate(all="ignore"):
            for r in range(3):
                p0 = (R[3 * r] * x).astype(F32)
                p1 = (R[3 * r + 1] * y).astype(F32)
                p2 = (R[3 * r + 2] * z).astype(F32)
                w[:, r] = (((p0 + p1).astype(F32) + p2).astype(F32) + t[r]).astype(F32)
        return np.isfinite(xyz).all(axis=1), w

    def bin(self, xyz, step):
        """Steps 1 .. 8 -> (takes_part bool, cell int64, k int64) of every record (cell and k are 0 where it takes no part)."""
        finite, w = self.world(xyz, step)
        origin = np.asarray(step, dtype=np.uint32)[12:15].view(F32)
        a, b, h = [(-w[:, abs(p) - 1] if p < 0 else w[:, abs(p) - 1]) for p in self.axes]   # a negation is exact
        with np.errstate(all="ignore"):
            va = ((a - origin[0]).astype(F32) * self.inv_c).astype(F32)
            vb = ((b - origin[1]).astype(F32) * self.inv_c).astype(F32)
            v = ((h - origin[2]).astype(F32) * self.inv_q).astype(F32)
            part = finite & (va >= F32(0.0)) & (va < F32(self.n_a)) & (vb >= F32(0.0)) & (vb < F32(self.n_b))
            part &= (v >= F32(-32767.0)) & (v <= F32(32767.0))
            ia = np.where(part, np.floor(va), 0).astype(np.int64)
            ib = np.where(part, np.floor(vb), 0).astype(np.int64)
            k = np.where(part, np.rint(v), 0).astype(np.int64)        # round half to even
        assert va.dtype == F32 and v.dtype == F32
        return part, np.where(part, ib * self.n_a + ia, 0), k

    # ---------------------------------------------------------------------------------------------------- per cell
    def cells(self, cell, k):
        """The moments and the six outputs from the cells and heights of the points that take part."""
        cell, k = np.asarray(cell, dtype=np.int64), np.asarray(k, dtype=np.int64)
        n = self.n_cells
        count = np.bincount(cell, minlength=n).astype(np.int64)
        total = np.zeros(n, dtype=np.int64)
        total2 = np.zeros(n, dtype=np.int64)                          # (below 2^62)
        np.add.at(total, cell, k)
        np.add.at(total2, cell, k * k)
        seen = count > 0
        m = np.where(seen, np.floor_divide(total, np.maximum(count, 1)), 0)      # floor division towards -inf
        dev = k - m[cell]
        S = np.zeros(n, dtype=np.uint64)
        np.add.at(S, cell, (dev * dev).astype(np.uint64))             # DIRECTLY: the sum of (k - m)^2
        spread = np.where(seen, S // np.maximum(count, 1).astype(np.uint64), EMPTY_SPREAD).astype(np.uint64)
        assert spread.max(initial=0) <= EMPTY_SPREAD
        flat = (count >= self.min_count) & (spread <= self.max_spread_q2)
        return dict(count=count.astype(np.uint32), sum=total, sum2=total2.astype(np.uint64),
                    mean_q=np.where(seen, m, -(1 << 31)).astype(np.int32), spread_q2=spread.astype(np.uint32), flat=flat.astype(np.uint8))

    # ---------------------------------------------------------------------------------------------------- sites
    def sites(self, mean_q, flat, allowed=None):
        """The direct window: uint8 x n_cells."""
        n_a, n_b, W = self.n_a, self.n_b, self.window
        mean = np.asarray(mean_q, dtype=np.int64).reshape(n_b, n_a)
        fl = np.asarray(flat).reshape(n_b, n_a) != 0
        site = np.zeros((n_b, n_a), dtype=bool)
        if n_a > 2 * W and n_b > 2 * W:
            inner = np.ones((n_b - 2 * W, n_a - 2 * W), dtype=bool)
            centre = mean[W:n_b - W, W:n_a - W]
            for dj in range(-W, W + 1):
                for di in range(-W, W + 1):
                    other = mean[W + dj:n_b - W + dj, W + di:n_a - W + di]
                    inner &= fl[W + dj:n_b - W + dj, W + di:n_a - W + di] & (np.abs(other - centre) <= self.max_step_q)
            site[W:n_b - W, W:n_a - W] = inner
        site = site.reshape(-1)
        if allowed is not None:
            site &= np.asarray(allowed).reshape(-1) != 0
        return site.astype(np.uint8)

    def cost(self, spread_q2, goal_i, goal_j):
        """The cost of every cell as if it were a site (uint64: no wrap to hide)."""
        j, i = np.divmod(np.arange(self.n_cells, dtype=np.int64), self.n_a)
        dist = (i - goal_i) ** 2 + (j - goal_j) ** 2 if goal_i < self.n_a and goal_j < self.n_b else 0 * i
        c = self.w_dist * dist + self.w_rough * np.minimum(np.asarray(spread_q2, dtype=np.int64), self.rough_cap)
        assert c.max(initial=0) < 0xFFFFFFFF
        return c.astype(np.uint64)

    def candidates(self, site, spread_q2, goal_i, goal_j, n_candidates):
        keys = (self.cost(spread_q2, goal_i, goal_j) << np.uint64(32)) | np.arange(self.n_cells, dtype=np.uint64)
        keys = np.sort(keys[np.asarray(site) != 0])[:n_candidates]
        out = np.full(n_candidates, NO_CANDIDATE, dtype=np.uint64)
        out[:len(keys)] = keys
        return out

    # ---------------------------------------------------------------------------------------------------- one call
    def process(self, xyz, step, allowed=None, n_candidates=1):
        """Every output of d2pc_sectors_ground_process_device for the records `xyz` (those the call visits, any order)."""
        step = np.asarray(step, dtype=np.uint32)
        part, cell, k = self.bin(xyz, step)
        out = self.cells(cell[part], k[part])
        out["site"] = self.sites(out["mean_q"], out["flat"], allowed)
        out["candidates"] = self.candidates(out["site"], out["spread_q2"], int(step[15]), int(step[16]), n_candidates)
        out["summary"] = np.array([int(out["count"].astype(np.uint64).sum()) & 0xFFFFFFFF, int(out["flat"].sum()), int(out["site"].sum()), 0],
                                  dtype=np.uint32)
        return out


def brute_sites(n_a, n_b, W, max_step_q, mean_q, flat, allowed=None):
    """The sites cell by cell, written independently of SectorsGroundRef.sites."""
    site = np.zeros(n_a * n_b, dtype=np.uint8)
    for j in range(n_b):
        for i in range(n_a):
            ok = allowed is None or allowed[j * n_a + i] != 0
            for dj in range(-W, W + 1):
                for di in range(-W, W + 1):
                    ii, jj = i + di, j + dj
                    if not (0 <= ii < n_a and 0 <= jj < n_b):
                        ok = False
                    elif not flat[jj * n_a + ii] or abs(int(mean_q[jj * n_a + ii]) - int(mean_q[j * n_a + i])) > max_step_q:
                        ok = False
            site[j * n_a + i] = 1 if ok else 0
    return site
