"""The TERRAIN block of include/d2pc_sectors.h restated in numpy and Python integers: the state block as the bytes the device
holds (16 headers, then `depth` tables in the ground slab's order), the anchor in float32 with one rounding per operation,
the ring and its header rules, the window summed with wrapping by masks, and tests/sectors_ground_ref.py for everything
behind the window's count, sum and sum2 (the sites, the cost, the candidates).  The per-cell formula is restated from
moments here (the ground's reference forms it from points): floor division and S by the wrapped formula in Python integers,
which tests/test_sectors_ground_cpu.py checks against the direct sum."""
import numpy as np

import sectors_ground_ref as gref

F32 = np.float32
MAX_DEPTH, HEADERS_BYTES = 16, 256
ANCHOR_MAX = F32(536870912.0)
M32, M64 = (1 << 32) - 1, (1 << 64) - 1


def slot_bytes(n_cells):
    return (20 * n_cells + 15) // 16 * 16


def anchor(step, inv_c):
    """Step 1 -> (anchored, ia0, jb0)."""
    o = np.asarray(step, dtype=np.uint32)[12:14].view(F32)
    with np.errstate(all="ignore"):
        ua, ub = F32(o[0] * F32(inv_c)), F32(o[1] * F32(inv_c))
        ok = bool(np.abs(ua) <= ANCHOR_MAX) and bool(np.abs(ub) <= ANCHOR_MAX)          # a NaN fails
    return (True, int(np.rint(ua)), int(np.rint(ub))) if ok else (False, 0, 0)           # rint: half to even


def cell_outputs(count, total, total2, min_count, max_spread_q2):
    """mean_q (int32), spread_q2 (uint32), flat (uint8) of cells whose count (uint32), sum and sum2 (uint64 words) are given:
    the wrapping formulas, entry by entry in Python integers."""
    n = len(count)
    mean, spread, flat = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint8)
    for c in range(n):
        cnt, s, s2 = int(count[c]), int(total[c]), int(total2[c])
        if cnt == 0:
            mean[c], spread[c] = gref.EMPTY_MEAN, gref.EMPTY_SPREAD
            continue
        signed = s - (1 << 64) if s >> 63 else s
        m = signed // cnt                                             # Python's floor division
        S = gref.wrapped_spread_sum(cnt, signed, s2, m)
        mean[c], spread[c] = m & M32, (S // cnt) & M32
        flat[c] = 1 if cnt >= min_count and int(spread[c]) <= max_spread_q2 else 0
    return mean.view(np.int32), spread, flat


class SectorsTerrainRef:
    def __init__(self, cfg, ground_geometry, depth):
        """cfg: the SectorsGroundConfig; ground_geometry: inv_c and inv_q (d2pc_sectors_ground_geometry's); depth: 1 .. 16."""
        self.g = gref.SectorsGroundRef(cfg, ground_geometry)
        self.n_a, self.n_b, self.n = self.g.n_a, self.g.n_b, self.g.n_cells
        self.depth, self.inv_c = int(depth), F32(ground_geometry.inv_c)
        self.slot_bytes = slot_bytes(self.n)
        self.state = np.zeros(HEADERS_BYTES + self.depth * self.slot_bytes, dtype=np.uint8)

    # ------------------------------------------------------------------------------------------------------- the state
    def headers(self):
        """uint32 (16, 4) view: ia0, jb0, the bits of h0, seq."""
        return self.state[:HEADERS_BYTES].view(np.uint32).reshape(MAX_DEPTH, 4)

    def table(self, s):
        """(sum uint64, sum2 uint64, count uint32) views of slot s."""
        base, n = HEADERS_BYTES + s * self.slot_bytes, self.n
        return (self.state[base:base + 8 * n].view(np.uint64), self.state[base + 8 * n:base + 16 * n].view(np.uint64),
                self.state[base + 16 * n:base + 20 * n].view(np.uint32))

    def reset(self):
        self.state[:HEADERS_BYTES] = 0

    # ------------------------------------------------------------------------------------------------------ one update
    def update(self, step, frame_count, frame_sum, frame_sum2, allowed=None, n_candidates=1):
        """Every output of d2pc_sectors_terrain_update_device, status included; the state moves as the device's does."""
        step = np.asarray(step, dtype=np.uint32)
        n, n_a, n_b = self.n, self.n_a, self.n_b
        fc = np.asarray(frame_count).astype(np.uint32)
        fs = np.ascontiguousarray(frame_sum).view(np.uint64) if np.asarray(frame_sum).dtype == np.int64 else np.asarray(frame_sum, dtype=np.uint64)
        fs2 = np.asarray(frame_sum2).astype(np.uint64)
        hdr = self.headers()
        anchored, ia0, jb0 = anchor(step, self.inv_c)
        seqs = [int(hdr[s, 3]) for s in range(self.depth)]
        count, total, total2 = np.zeros(n, dtype=np.uint32), np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint64)
        if not anchored:
            status = [max(seqs), 0, 0, 0]
        else:
            if max(seqs) == M32:                                      # all slots are first taken as empty
                hdr[:self.depth] = 0
                seqs = [0] * self.depth
            v = seqs.index(min(seqs))                                 # the lowest index on a tie
            q = max(seqs) + 1
            h0 = step[14:15].view(F32)[0]
            took = 1
            count, total, total2 = fc.copy(), fs.copy(), fs2.copy()
            j, i = np.divmod(np.arange(n, dtype=np.int64), n_a)
            for s in range(self.depth):
                if s == v or seqs[s] == 0 or not (hdr[s, 2:3].view(F32)[0] == h0):        # float ==: a NaN matches nothing
                    continue
                di, dj = ia0 - int(hdr[s, 0:1].view(np.int32)[0]), jb0 - int(hdr[s, 1:2].view(np.int32)[0])   # Python integers
                ii, jj = i + di, j + dj
                inside = (ii >= 0) & (ii < n_a) & (jj >= 0) & (jj < n_b)
                if not inside.any():
                    continue                                          # the shift leaves the grid: the slot takes no part
                took += 1
                t_sum, t_sum2, t_count = self.table(s)
                o = (jj * n_a + ii)[inside]
                with np.errstate(over="ignore"):
                    count[inside] += t_count[o]                       # modulo 2^32
                    total[inside] += t_sum[o]                         # modulo 2^64
                    total2[inside] += t_sum2[o]
            hdr[v] = [ia0 & M32, jb0 & M32, int(step[14]), q]
            t_sum, t_sum2, t_count = self.table(v)
            t_sum[:], t_sum2[:], t_count[:] = fs, fs2, fc
            status = [q, took, ia0 & M32, jb0 & M32]
        mean, spread, flat = cell_outputs(count, total, total2, self.g.min_count, self.g.max_spread_q2)
        site = self.g.sites(mean, flat, allowed)
        return dict(count=count, sum=total.view(np.int64), sum2=total2, mean_q=mean, spread_q2=spread, flat=flat, site=site,
                    candidates=self.g.candidates(site, spread, int(step[15]), int(step[16]), n_candidates),
                    summary=np.array([int(count.astype(np.uint64).sum()) & M32, int(flat.sum()), int(site.sum()), 0], dtype=np.uint32),
                    status=np.array(status, dtype=np.uint64).astype(np.uint32))
