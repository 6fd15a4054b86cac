"""The RELIEF block of include/d2pc_sectors.h restated in numpy and Python integers: the state block as the bytes the device
holds (16 headers, then `depth` tables in the slope slab's order: nine 64-bit planes, then the counts), the ring and the
window of tests/sectors_terrain_ref.py over ten sums (its anchor IS that file's), and the SLOPE block's fit restated FROM
SUMS: the floor mean and the wrapped S = sum2 - 2 m sum + N m^2 in Python integers modulo 2^64, the pre-steps likewise, then
the double sequence one numpy float64 operation at a time (numpy contracts nothing).  tests/sectors_slope_ref.py forms the
same outputs from points, with S summed directly; tests/test_sectors_relief_cpu.py holds the two against each other.  The
sites, the cost and the candidates are tests/sectors_ground_ref.py's."""
import numpy as np

import sectors_ground_ref as gref
import sectors_slope_ref as sref
import sectors_terrain_ref as tref

F32, F64 = np.float32, np.float64
MAX_DEPTH, HEADERS_BYTES = 16, 256
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
WORDS = 9                                       # the 64-bit planes: sum, sum2, su, sw, suu, suw, sww, suk, swk
OUT = sref.OUT + ("status",)
DTYPE = dict(sref.DTYPE, status=np.uint32)


def slot_bytes(n_cells):
    return (76 * n_cells + 15) // 16 * 16


def signed64(x):
    x &= M64
    return x - (1 << 64) if x >> 63 else x


def frame_planes(frame_sum, frame_sum2, frame_moments, n):
    """The nine planes (9, n) uint64 of a frame's sum, sum2 and moments as a slope call wrote them."""
    p = np.zeros((WORDS, n), dtype=np.uint64)
    p[0] = np.ascontiguousarray(frame_sum).view(np.uint64) if np.asarray(frame_sum).dtype == np.int64 else np.asarray(frame_sum, dtype=np.uint64)
    p[1] = np.asarray(frame_sum2).astype(np.uint64)
    m = np.ascontiguousarray(frame_moments)
    p[2:] = (m.view(np.uint64) if m.dtype == np.int64 else m.astype(np.uint64)).reshape(7, n)
    return p


def fit_from_sums(count, planes, min_fit, max_spread_q2, scale, max_tilt2):
    """The SLOPE block's fit and per-cell outputs of cells whose count (uint32) and nine sums (uint64 words, (9, n)) are given.
    The integer steps cell by cell in Python integers, wrapping by masks; every value then goes to float64 on its own (Python
    rounds an integer to the nearest double, ties to even), and the double sequence is one numpy operation at a time."""
    n = len(count)
    mean, spread = np.full(n, sref.EMPTY_LEVEL, dtype=np.uint32), np.full(n, sref.EMPTY_RESID, dtype=np.uint32)
    cols = {k: np.zeros(n, dtype=F64) for k in ("N", "S", "r", "su", "sw", "suu", "suw", "sww", "suk", "swk")}
    for c in np.flatnonzero(count):
        cnt = int(count[c])
        s = [int(x) for x in planes[:, c]]
        m = signed64(s[0]) // cnt                                     # Python's floor division
        S = (s[1] - 2 * m * s[0] + cnt * m * m) & M64                 # wrapping
        mean[c], spread[c] = m & M32, (S // cnt) & M32
        m = (m & M32) - (1 << 32) if (m & M32) >> 31 else m & M32      # the pre-steps widen the 32-bit mean again (the same m for |m| < 2^31)
        vals = dict(N=cnt, S=(s[1] - 2 * m * s[0] + cnt * m * m) & M64, r=signed64(s[0] - cnt * m), su=signed64(s[2]), sw=signed64(s[3]),
                    suu=signed64(s[4]), suw=signed64(s[5]), sww=signed64(s[6]), suk=signed64(s[7] - m * s[2]), swk=signed64(s[8] - m * s[3]))
        for k, v in vals.items():
            cols[k][c] = float(v)
    seen = np.asarray(count) != 0
    N, SS, rr, su, sw, suu, suw, sww, suk, swk = [cols[k] for k in ("N", "S", "r", "su", "sw", "suu", "suw", "sww", "suk", "swk")]
    with np.errstate(all="ignore"):
        A, B, C = N * suu - su * su, N * suw - su * sw, N * sww - sw * sw
        E, F, G = N * suk - su * rr, N * swk - sw * rr, N * SS - rr * rr
        AC = A * C
        D = AC - B * B
        fitted = seen & (np.asarray(count) >= min_fit) & (AC > 0.0) & (D * 1048576.0 > AC)
        gu, gw = (E * C - F * B) / D, (F * A - E * B) / D
        Q = (G - gu * E) - gw * F
        c0 = ((rr - gu * su) - gw * sw) / N
        sa, sb = gu * F64(scale), gw * F64(scale)
        rc = np.clip(np.rint(np.where(fitted, c0, 0.0)), -2147483648.0, 2147483647.0).astype(np.int64)      # rint: half to even
        mq = np.floor(np.where(Q > 0.0, Q, 0.0) / (N * N))
        resid_fit = np.where(mq >= 4294967294.0, F64(0xFFFFFFFE), np.where(fitted, mq, 0.0)).astype(np.uint64)
        tilt_ok = sa * sa + sb * sb <= F64(max_tilt2)
        slope_a = np.where(fitted, sa.astype(F32).view(np.uint32), np.uint32(sref.NOT_FITTED)).astype(np.uint32)
        slope_b = np.where(fitted, sb.astype(F32).view(np.uint32), np.uint32(sref.NOT_FITTED)).astype(np.uint32)
    assert A.dtype == F64 and c0.dtype == F64 and sa.dtype == F64
    level = np.where(fitted, (mean.astype(np.int64) + rc) & M32, mean).astype(np.uint32).view(np.int32)
    resid = np.where(fitted, resid_fit, spread).astype(np.uint32)
    flat = fitted & (resid <= max_spread_q2) & tilt_ok
    return dict(slope_a=slope_a, slope_b=slope_b, level_q=level, resid_q2=resid, flat=flat.astype(np.uint8), fitted=fitted)


class SectorsReliefRef:
    def __init__(self, cfg, scfg, geometry, depth):
        """cfg: a SectorsGroundConfig; scfg: a SectorsSlopeConfig (or anything with their fields); geometry: inv_c, inv_q
        (d2pc_sectors_ground_geometry's); depth: 1 .. 16."""
        self.slope = sref.SectorsSlopeRef(cfg, scfg, geometry)
        self.g = self.slope.ground
        self.n_a, self.n_b, self.n = self.g.n_a, self.g.n_b, self.g.n_cells
        self.depth, self.inv_c = int(depth), F32(geometry.inv_c)
        self.slot_bytes = slot_bytes(self.n)
        self.state = np.zeros(HEADERS_BYTES + self.depth * self.slot_bytes, dtype=np.uint8)

    # ------------------------------------------------------------------------------------------------------- the state
    def headers(self):
        """uint32 (16, 4) view: ia0, jb0, the bits of h0, seq."""
        return self.state[:HEADERS_BYTES].view(np.uint32).reshape(MAX_DEPTH, 4)

    def table(self, s):
        """(the nine planes uint64 (9, n), count uint32) views of slot s."""
        base, n = HEADERS_BYTES + s * self.slot_bytes, self.n
        return (self.state[base:base + 72 * n].view(np.uint64).reshape(WORDS, n), self.state[base + 72 * n:base + 76 * n].view(np.uint32))

    def reset(self):
        self.state[:HEADERS_BYTES] = 0

    # ------------------------------------------------------------------------------------------------------ one update
    def window(self, step, fc, fp):
        """Steps 1 .. 4 and 6: (count, planes, status) of the window; the state moves as the device's does."""
        n, n_a, n_b = self.n, self.n_a, self.n_b
        hdr = self.headers()
        anchored, ia0, jb0 = tref.anchor(step, self.inv_c)
        seqs = [int(hdr[s, 3]) for s in range(self.depth)]
        if not anchored:
            return np.zeros(n, dtype=np.uint32), np.zeros((WORDS, n), dtype=np.uint64), [max(seqs), 0, 0, 0]
        if max(seqs) == M32:                                          # all slots are first taken as empty
            hdr[:self.depth] = 0
            seqs = [0] * self.depth
        v = seqs.index(min(seqs))                                     # the lowest index on a tie
        q = max(seqs) + 1
        h0 = step[14:15].view(F32)[0]
        took = 1
        count, planes = fc.copy(), fp.copy()
        j, i = np.divmod(np.arange(n, dtype=np.int64), n_a)
        for s in range(self.depth):
            if s == v or seqs[s] == 0 or not (hdr[s, 2:3].view(F32)[0] == h0):            # float ==: a NaN matches nothing
                continue
            di, dj = ia0 - int(hdr[s, 0:1].view(np.int32)[0]), jb0 - int(hdr[s, 1:2].view(np.int32)[0])       # Python integers
            ii, jj = i + di, j + dj
            inside = (ii >= 0) & (ii < n_a) & (jj >= 0) & (jj < n_b)
            if not inside.any():
                continue                                              # the shift leaves the grid: the slot takes no part
            took += 1
            t_planes, t_count = self.table(s)
            o = (jj * n_a + ii)[inside]
            with np.errstate(over="ignore"):
                count[inside] += t_count[o]                           # modulo 2^32
                planes[:, inside] += t_planes[:, o]                   # modulo 2^64
        hdr[v] = [ia0 & M32, jb0 & M32, int(step[14]), q]
        t_planes, t_count = self.table(v)
        t_planes[:], t_count[:] = fp, fc
        return count, planes, [q, took, ia0 & M32, jb0 & M32]

    def update(self, step, frame_count, frame_sum, frame_sum2, frame_moments, allowed=None, n_candidates=1):
        """Every output of d2pc_sectors_relief_update_device, status included, and `fitted` beside them; the slopes as bits."""
        step = np.asarray(step, dtype=np.uint32)
        fc = np.asarray(frame_count).astype(np.uint32)
        fp = frame_planes(frame_sum, frame_sum2, frame_moments, self.n)
        count, planes, status = self.window(step, fc, fp)
        out = fit_from_sums(count, planes, self.slope.min_fit, self.slope.max_spread_q2, self.slope.scale, self.slope.max_tilt2)
        out.update(count=count, sum=planes[0].view(np.int64).copy(), sum2=planes[1].copy(), moments=planes[2:].reshape(-1).view(np.int64).copy())
        out["site"] = self.g.sites(out["level_q"], out["flat"], allowed)
        out["candidates"] = self.g.candidates(out["site"], out["resid_q2"], int(step[15]), int(step[16]), n_candidates)
        out["summary"] = np.array([int(count.astype(np.uint64).sum()) & M32, int(out["flat"].sum()), int(out["site"].sum()),
                                   int(out["fitted"].sum())], dtype=np.uint32)
        out["status"] = np.array(status, dtype=np.uint64).astype(np.uint32)
        return out
