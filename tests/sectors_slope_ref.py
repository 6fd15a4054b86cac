"""The SLOPE block of include/d2pc_sectors.h restated in numpy: float32 with an explicit astype after every operation for
steps 1 .. 9 (one rounding per operation, nothing fused), int64 for the ten sums and the wrapping pre-steps, float64 element
by element for the fit (one ufunc per operation: numpy contracts nothing).  S is computed DIRECTLY as the sum of (k - m)^2,
not by the wrapped formula the kernel uses, as tests/sectors_ground_ref.py does; the sites, the cost and the candidates ARE
that file's.  inv_c and inv_q are ARGUMENTS (the library's own, d2pc_sectors_ground_geometry); scale and max_tilt2 are formed
here, in Python floats, and the tests compare them with d2pc_sectors_slope_geometry's."""
import numpy as np

import sectors_ground_ref as gref

F32 = np.float32
NOT_FITTED = 0x7FC00000
EMPTY_LEVEL, EMPTY_RESID = 0x80000000, 0xFFFFFFFF
MOMENTS = ("su", "sw", "suu", "suw", "sww", "suk", "swk")
OUT = ("count", "sum", "sum2", "moments", "slope_a", "slope_b", "level_q", "resid_q2", "flat", "site", "candidates", "summary")
DTYPE = dict(count=np.uint32, sum=np.int64, sum2=np.uint64, moments=np.int64, slope_a=np.uint32, slope_b=np.uint32, level_q=np.int32,
             resid_q2=np.uint32, flat=np.uint8, site=np.uint8, candidates=np.uint64, summary=np.uint32)     # (the slopes as bits)

step_words, rotation = gref.step_words, gref.rotation


def scale_of(quantum, cell_size, sub):
    """scale = (double)quantum * (2 P) / (double)cell_size, of the float32 fields."""
    return float(F32(quantum)) * float(2 * sub) / float(F32(cell_size))


def max_tilt2_of(max_slope):
    return float(F32(max_slope)) * float(F32(max_slope))


class SectorsSlopeRef:
    def __init__(self, cfg, scfg, geometry):
        """cfg: a SectorsGroundConfig; scfg: a SectorsSlopeConfig (or anything with their fields); geometry: inv_c, inv_q."""
        self.ground = gref.SectorsGroundRef(cfg, geometry)
        self.n_a, self.n_b, self.n_cells = self.ground.n_a, self.ground.n_b, self.ground.n_cells
        self.sub = int(scfg.sub)
        self.scale = scale_of(cfg.quantum, cfg.cell_size, self.sub)
        self.max_tilt2 = max_tilt2_of(scfg.max_slope)
        self.min_fit = max(int(cfg.min_count), 3)
        self.max_spread_q2 = int(cfg.max_spread_q2)

    # ---------------------------------------------------------------------------------------------------- per record
    def bin(self, xyz, step):
        """Steps 1 .. 9 -> (takes_part bool, cell, k, u, w as int64) of every record (zeros where it takes no part)."""
        g = self.ground
        finite, wld = g.world(xyz, step)
        origin = np.asarray(step, dtype=np.uint32)[12:15].view(F32)
        a, b, h = [(-wld[:, abs(p) - 1] if p < 0 else wld[:, abs(p) - 1]) for p in g.axes]   # a negation is exact
        P = F32(self.sub)
        with np.errstate(all="ignore"):
            va = ((a - origin[0]).astype(F32) * g.inv_c).astype(F32)
            vb = ((b - origin[1]).astype(F32) * g.inv_c).astype(F32)
            v = ((h - origin[2]).astype(F32) * g.inv_q).astype(F32)
            part = finite & (va >= F32(0.0)) & (va < F32(g.n_a)) & (vb >= F32(0.0)) & (vb < F32(g.n_b))
            part &= (v >= F32(-32767.0)) & (v <= F32(32767.0))
            va, vb, v = np.where(part, va, F32(0)), np.where(part, vb, F32(0)), np.where(part, v, F32(0))
            ia, ib = np.floor(va).astype(np.int64), np.floor(vb).astype(np.int64)
            k = np.rint(v).astype(np.int64)                                # round half to even
            fa, fb = (va - np.floor(va)).astype(F32), (vb - np.floor(vb)).astype(F32)
            pa, pb = np.floor((fa * P).astype(F32)).astype(np.int64), np.floor((fb * P).astype(F32)).astype(np.int64)
        assert va.dtype == F32 and fa.dtype == F32 and (fa * P).dtype == F32
        u, w = 2 * pa - (self.sub - 1), 2 * pb - (self.sub - 1)
        z = np.int64(0)
        return part, np.where(part, ib * g.n_a + ia, z), k, np.where(part, u, z), np.where(part, w, z)

    # ---------------------------------------------------------------------------------------------------- per cell
    def cells(self, cell, k, u, w):
        """The ten sums and the per-cell outputs from the points that take part."""
        cell, k, u, w = [np.asarray(x, dtype=np.int64) for x in (cell, k, u, w)]
        n = self.n_cells
        assert np.all(np.abs(u) < self.sub) and np.all(u % 2 != 0) and np.all(np.abs(w) < self.sub) and np.all(w % 2 != 0)

        def total(term):
            t = np.zeros(n, dtype=np.int64)
            np.add.at(t, cell, term)
            return t

        count = np.bincount(cell, minlength=n).astype(np.int64)
        s1, s2 = total(k), total(k * k)
        mom = dict(su=total(u), sw=total(w), suu=total(u * u), suw=total(u * w), sww=total(w * w), suk=total(u * k), swk=total(w * k))
        seen = count > 0
        m = np.where(seen, np.floor_divide(s1, np.maximum(count, 1)), 0)            # floor division towards -inf
        dev = k - m[cell]
        S = np.zeros(n, dtype=np.uint64)
        np.add.at(S, cell, (dev * dev).astype(np.uint64))                           # DIRECTLY: the sum of (k - m)^2
        spread = np.where(seen, S // np.maximum(count, 1).astype(np.uint64), EMPTY_RESID).astype(np.uint64)
        # the integer pre-steps (int64 wraps as the device's does; nothing here comes near)
        r = s1 - count * m
        suk1, swk1 = mom["suk"] - m * mom["su"], mom["swk"] - m * mom["sw"]
        f64 = np.float64
        N, su, sw, suu, suw, sww = [x.astype(f64) for x in (count, mom["su"], mom["sw"], mom["suu"], mom["suw"], mom["sww"])]
        suk, swk, rr, SS = suk1.astype(f64), swk1.astype(f64), r.astype(f64), S.astype(f64)
        with np.errstate(all="ignore"):
            A, B, C = N * suu - su * su, N * suw - su * sw, N * sww - sw * sw
            E, F, G = N * suk - su * rr, N * swk - sw * rr, N * SS - rr * rr
            AC = A * C
            D = AC - B * B
            fitted = (count >= self.min_fit) & (AC > 0.0) & (D * 1048576.0 > AC)
            gu, gw = (E * C - F * B) / D, (F * A - E * B) / D
            Q = (G - gu * E) - gw * F
            c0 = ((rr - gu * su) - gw * sw) / N
            sa, sb = gu * self.scale, gw * self.scale
            rc = np.clip(np.rint(np.where(fitted, c0, 0.0)), -2147483648.0, 2147483647.0).astype(np.int64)
            mq = np.floor(np.where(Q > 0.0, Q, 0.0) / (N * N))
            resid_fit = np.where(mq >= 4294967294.0, f64(0xFFFFFFFE), np.where(fitted, mq, 0.0)).astype(np.uint64)
            tilt_ok = sa * sa + sb * sb <= self.max_tilt2
            slope_a = np.where(fitted, sa.astype(F32).view(np.uint32), np.uint32(NOT_FITTED)).astype(np.uint32)
            slope_b = np.where(fitted, sb.astype(F32).view(np.uint32), np.uint32(NOT_FITTED)).astype(np.uint32)
        assert A.dtype == f64 and c0.dtype == f64
        level = np.where(fitted, (m + rc) & 0xFFFFFFFF, np.where(seen, m & 0xFFFFFFFF, EMPTY_LEVEL)).astype(np.uint32).view(np.int32)
        resid = np.where(fitted, resid_fit, spread).astype(np.uint32)
        flat = fitted & (resid <= self.max_spread_q2) & tilt_ok
        return dict(count=count.astype(np.uint32), sum=s1, sum2=s2.astype(np.uint64), moments=np.concatenate([mom[x] for x in MOMENTS]),
                    slope_a=slope_a, slope_b=slope_b, level_q=level, resid_q2=resid, flat=flat.astype(np.uint8), fitted=fitted)

    # ---------------------------------------------------------------------------------------------------- one call
    def process(self, xyz, step, allowed=None, n_candidates=1):
        """Every output of d2pc_sectors_slope_process_device for the records `xyz` (those the call visits, any order); the
        slopes as their bits; `fitted` beside them."""
        step = np.asarray(step, dtype=np.uint32)
        part, cell, k, u, w = self.bin(xyz, step)
        out = self.cells(cell[part], k[part], u[part], w[part])
        g = self.ground
        out["site"] = g.sites(out["level_q"], out["flat"], allowed)
        out["candidates"] = g.candidates(out["site"], out["resid_q2"], int(step[15]), int(step[16]), n_candidates)
        out["summary"] = np.array([int(out["count"].astype(np.uint64).sum()) & 0xFFFFFFFF, int(out["flat"].sum()), int(out["site"].sum()),
                                   int(out["fitted"].sum())], dtype=np.uint32)
        return out


def as_float(bits):
    return np.asarray(bits, dtype=np.uint32).view(F32)
