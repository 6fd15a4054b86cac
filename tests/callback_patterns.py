"""Built inputs for the fused COMPACT callback kernels (d2pc_callback.hip) and a numpy model of their hand-off.

Those kernels place survivors by their own structure, not by the runs / slots / groups that occupancy_patterns.py
attacks: per-row counts of a 256 x 32 tile, two 9-bit counts and a tag per published dword, lane 16 j + p summing the
tiles j, j + 4, ... of a band, "left of the tile" sums, band accumulators summed 64 per step, a fast count that takes 4
consecutive bytes per lane and a scatter that walks 64-column steps.  Their input goes through the k x k median first,
so a pattern here is a u8 FRAME (ROI, border and the ring outside the filter's reach) together with k, and the survivors
are whatever the median leaves: the expected answer is always np.flatnonzero of

    valid = (oracle.median_u8(frame, k)[ROI] * scale > dmin) & (W != 0)

(`Pattern.valid`), never the model below.  The median commutes with thresholding, so a frame is a two-level seed B
(`hi` bytes drawn above the floor, `lo` = 0 or bytes at and below the floor byte, the floor byte itself among them)
and the mask is the k x k binary median of B.  Seeds whose median is known in closed form:

  plus (k = 3)        5 pixels, exactly one survivor at the centre
  run  (k = 3)        L pixels in row r from x0, row r - 1 where (x - x0) % 3 == 0, row r + 1 where (x - x0) % 3 == 1:
                      L - 2 survivors in row r alone, from x0 + 1
  run  (k = 11)       rows r - 5, r + 5, r - 1, r, r + 1 over [x0, x0 + L), row r - 3 where (x - x0) % 11 < 6:
                      L - 10 survivors in row r alone, from x0 + 5; such rows lie 11 apart, 15 where they share columns
  rectangle (any k)   straight edges survive, corners erode: one that spans a tile's columns exactly and reaches
                      (k + 1) / 2 rows beyond it fills the tile with 256 per row and leaves its neighbours in the band
                      empty; one that reaches (k + 1) / 2 beyond the tile sideways has full first and last rows, so its
                      vertical placement sets the parity of the first full row; an edge at tile column 254 gives 255

What each generator reaches is asserted on the oracle's median in tests/test_callback_patterns.py at the cases
tests/test_callback_compact_occupancy_gpu.py runs."""
import functools

import numpy as np

import oracle

TW, TH, STEP, GROUP, PAIR = 256, 32, 64, 4, 2       # tile, 64-column step of the scatter, bytes per lane of the fast count, rows per dword
BORDER = {3: 3, 11: 40}
SCALE = 0.125
FLOOR_BYTE = 97                                      # holes of kind "floor": bytes 0..97, dmin = 97 * 0.125 exactly
HOLES = ("zero", "floor")
FINE_COUNTS = (0, 1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255, 256)
COARSE_COUNTS = (0, 1, 2, 63, 64, 65, 128, 255, 256)     # k = 11: a run row every 15 rows leaves room for these
ROW_PAIRS = ((0, 256), (256, 0), (256, 256), (255, 256), (1, 0), (0, 1))
# tile rows of the ramp's runs: (rows every tile uses, the row a narrow last tile uses -- not the band's last occupied row:
# a narrow tile left out of a row's total must move the rows below it)
RAMP_ROWS = {3: ((2, 20, 27), 9), 11: ((19,), 4)}
RAMP_MUL, RAMP_MOD = 2654435761, 13
# Rows of runs that share columns: at k = 11 a window over the last seed row of one run and the first five of the next
# holds 61 set pixels from a distance of 14 rows down, so 11 apart is not enough there; ODD_GAP alternates the row parity.
GAP, ODD_GAP = {3: 4, 11: 15}, {3: 5, 11: 17}
SHAPES = {"five": (1031, 250), "five_odd": (1031, 249), "sixteen": (4096, 96), "seventeen": (4097, 96),
          "tall": (256, 4160), "tall2": (257, 4160), "taller": (256, 6400), "taller2": (257, 6400), "small3": (672, 400)}
GENERATORS = ("row_counts", "step_only", "edges", "tile_steps", "empty_bands", "tile_ramp")
SLIPS = ("count_8bit", "pair_swapped", "left_includes_self", "left_first_16_tiles", "above_first_64", "above_first_128",
         "tail_cols_counted", "tail_rows_counted", "group_not_clipped", "step_rank_restarts", "band_total_for_count")


def dmin_of(holes):
    return -np.inf if holes == "zero" else FLOOR_BYTE * SCALE


def tiles(roi_w, roi_h):
    return -(-roi_w // TW), -(-roi_h // TH)


def ramp_count(t):
    return 1 + (t * RAMP_MUL) % RAMP_MOD


# ------------------------------------------------------------------------------------------------------------------ seeds
class Canvas:
    """A two-level seed over the frame, addressed in ROI coordinates (negative ones and those past the ROI lie in the
    border).  The ring farther than k // 2 from the ROI is set from the start: it cannot move a ROI median, and it
    gives the columns and rows a tile has beyond a ragged ROI something that a count without its clip would find."""

    def __init__(self, roi_w, roi_h, k):
        self.roi_w, self.roi_h, self.k, self.b = roi_w, roi_h, k, BORDER[k]
        self.tx, self.ty = tiles(roi_w, roi_h)
        self.B = np.ones((roi_h + 2 * self.b, roi_w + 2 * self.b), dtype=bool)
        g = self.b - k // 2
        self.B[g:-g, g:-g] = False

    def width(self, tx):
        return min(TW, self.roi_w - TW * tx)

    def rect(self, x0, y0, x1, y1):
        b = self.b
        self.B[max(y0 + b, 0):max(y1 + b, 0), max(x0 + b, 0):max(x1 + b, 0)] = True

    def dots(self, y, x0, n, period, lo, hi):
        x = np.arange(x0, x0 + n)
        x = x[((x - x0) % period >= lo) & ((x - x0) % period < hi)] + self.b
        x = x[(x >= 0) & (x < self.B.shape[1])]
        if 0 <= y + self.b < self.B.shape[0]:
            self.B[y + self.b, x] = True

    def run(self, y, xs, c):
        """c >= 1 survivors in row y from column xs, none in the rows around it."""
        if self.k == 3:
            x0, n = xs - 1, c + 2
            self.rect(x0, y, x0 + n, y + 1)
            self.dots(y - 1, x0, n, 3, 0, 1)
            self.dots(y + 1, x0, n, 3, 1, 2)
        else:
            x0, n = xs - 5, c + 10
            for r in (y - 5, y + 5, y - 1, y, y + 1):
                self.rect(x0, r, x0 + n, r + 1)
            self.dots(y - 3, x0, n, 11, 0, 6)

    def single(self, x, y):
        if self.k == 3:      # the plus
            self.rect(x - 1, y, x + 2, y + 1)
            self.rect(x, y - 1, x + 1, y + 2)
        else:
            self.run(y, x, 1)

    def full_tile(self, tx, ty):
        # (the band's last tile goes on through the border: a ragged one may be a single column wide)
        m = (self.k + 1) // 2
        x1 = TW * tx + TW if tx < self.tx - 1 else self.roi_w + self.b
        self.rect(TW * tx, TH * ty - m, x1, min(TH * ty + TH, self.roi_h) + m)

    def ramp_tile(self, tx, ty):
        """ramp_count(t) survivors in each ramp row of tile t = ty * tiles_x + tx, at a start column of its own, six
        columns and more from the tile's edges (the seeds stay inside the tile).  A last tile narrower than 32 columns
        holds min(width, ramp_count) survivors up to the ROI's last column in the narrow row, which its left neighbour
        leaves free."""
        t = ty * self.tx + tx
        c, w = ramp_count(t), self.width(tx)
        rows, narrow_row = RAMP_ROWS[self.k]
        narrow_last = self.width(self.tx - 1) < 32
        if w < 32:
            y = TH * ty + narrow_row
            if y < self.roi_h:
                self.run(y, self.roi_w - min(w, c), min(w, c))
            return
        xs = TW * tx + 6 + (t * 37) % (w - RAMP_MOD - 11)
        for r in rows + (() if narrow_last and tx == self.tx - 2 else (narrow_row,)):
            if TH * ty + r < self.roi_h:
                self.run(TH * ty + r, xs, c)


def ramp_rows_of(roi_w, k, tx):
    """The tile rows in which tile column tx holds its ramp count (see Canvas.ramp_tile)."""
    ntx = -(-roi_w // TW)
    last_w = roi_w - TW * (ntx - 1)
    rows, narrow_row = RAMP_ROWS[k]
    if tx == ntx - 1 and last_w < 32:
        return (narrow_row,)
    return rows + (() if last_w < 32 and tx == ntx - 2 else (narrow_row,))


def _place_runs(cv, items, columns, y_start, rng):
    """One run per row: items (count, row parity) go to the next row of that parity at least GAP[k] below the last one
    of their tile column; the start column is seeded (0 for 256, 0 / 1 for 255)."""
    gap = GAP[cv.k]
    nxt = {tx: y_start for tx in columns}
    for j, (c, parity) in enumerate(items):
        tx = columns[j % len(columns)]
        y = nxt[tx] + (nxt[tx] + parity) % 2
        assert y < cv.roi_h, "the frame has too few rows for the listed runs"
        xs = int(rng.integers(0, TW - c + 1))
        cv.run(y, TW * tx + xs, c)
        nxt[tx] = y + gap


def row_counts(roi_w, roi_h, k, seed):
    """Rows 1..14 of one tile full (first full row odd, last even: the pairs (0, 256), (256, 256), (256, 0)); an L whose
    upper part ends at tile column 254 and whose lower part passes the tile: 255 per row, then 256 from an odd row on
    (the pair (255, 256)); below them one run per row with every listed count on an even and on an odd tile row."""
    out = []
    for s in range(2):
        cv = Canvas(roi_w, roi_h, k)
        rng = np.random.default_rng(1000 * seed + s)
        m, full = (k + 1) // 2, roi_w // TW
        ta, tl = (1, 3) if full >= 4 else (0, 1)
        cv.rect(TW * ta - m, 1, TW * ta + TW + m, 15)
        cv.rect(TW * tl - m, 26, TW * tl + 255, 38)
        cv.rect(TW * tl - m, 38, TW * tl + TW + m, 50)
        counts = [c for c in (FINE_COUNTS if k == 3 else COARSE_COUNTS) if c]
        items = [(c, p) for c in counts for p in (0, 1)]
        order = rng.permutation(len(items))
        _place_runs(cv, [items[i] for i in order], (0, 2) if full >= 3 else (0,), 50 + 3 * (k // 2) + 1, rng)
        out.append((f"s{s}", cv.B))
    return out


STEP_ONLY_SINGLES = (64, 127, 191, 192, 100, 101, 102, 103)   # step columns 0 and 63; every position of a 4-byte group


def step_only(roi_w, roi_h, k, seed):
    """One tile row at a time: 64 survivors that fill exactly one of the four 64-column steps; one survivor alone on a
    step's column 0 or 63; one survivor alone in each position of a 4-byte group."""
    out = []
    for s, tx in enumerate((1, 3)):
        cv = Canvas(roi_w, roi_h, k)
        y, gap = 2 + s, ODD_GAP[k]
        for q in range(4):
            cv.run(y, TW * tx + STEP * q, STEP)
            y += gap
        for x in STEP_ONLY_SINGLES:
            cv.single(TW * tx + x, y)
            y += gap
        assert y - gap < roi_h
        out.append((f"t{tx}", cv.B))
    return out


EDGE_FRAMES = ("cols", "first_row", "last_row", "first_px", "last_px", "none", "full")


def edge_columns(roi_w):
    full = roi_w // TW
    return sorted({0, TW - 1, TW, TW * full - 1, roi_w - 1})


def edges(roi_w, roi_h, k, seed):
    out = []
    for name in EDGE_FRAMES:
        cv = Canvas(roi_w, roi_h, k)
        if name == "cols":        # a tile row's only survivor in a tile's first column, in its last, in the ROI's last
            for i, x in enumerate(edge_columns(roi_w)):
                cv.single(x, 3 + i * ODD_GAP[k])
        elif name in ("first_row", "last_row"):
            y = 0 if name == "first_row" else roi_h - 1
            for tx in range(cv.tx):
                if cv.width(tx) >= 64:
                    cv.run(y, TW * tx + 20 + tx, 17 + tx)
        elif name == "first_px":
            cv.single(0, 0)
        elif name == "last_px":
            cv.single(roi_w - 1, roi_h - 1)
        elif name == "full":
            cv.B[:] = True
        out.append((name, cv.B))
    return out


def step_plan(roi_w, roi_h):
    """-> two frames of {band: [(first full tile, N empty tiles), ...]}; the chains lie in bands that are no neighbours,
    because a full tile reaches (k + 1) / 2 rows into the bands above and below it."""
    ntx, nty = tiles(roi_w, roi_h)
    if ntx >= 16:
        far = ntx - 7                   # (17 across: the chain ends on the one-column tile 16)
        return [{0: [(0, 1), (2, 3), (far, 5)], 2: [(1, 4)]}, {2: [(0, 1), (2, 3), (far, 5)], 0: [(1, 4)]}]
    assert ntx == 5 and nty >= 6
    return [{1: [(0, 1)], 4: [(0, 3)]}, {5: [(2, 1)], 2: [(0, 3)]}]


def tile_steps(roi_w, roi_h, k, seed):
    """Inside a band: a full tile, N empty tiles, a full tile; every other tile holds its ramp count."""
    out = []
    for s, plan in enumerate(step_plan(roi_w, roi_h)):
        cv = Canvas(roi_w, roi_h, k)
        fulls, empties = set(), set()
        for band, chains in plan.items():
            for a, n in chains:
                fulls |= {(a, band), (a + n + 1, band)}
                empties |= {(x, band) for x in range(a + 1, a + n + 1)}
        for ty in range(cv.ty):
            for tx in range(cv.tx):
                if (tx, ty) in fulls:
                    cv.full_tile(tx, ty)
                elif (tx, ty) not in empties and not (cv.width(tx) < 32 and {(tx, ty - 1), (tx, ty + 1)} & fulls):
                    cv.ramp_tile(tx, ty)     # (not a narrow tile below or above a full one: its run would meet the rows that reaches over)
        out.append((f"p{s}", cv.B))
    return out


def occupied_bands(roi_h):
    """-> two frames of occupied bands: whole empty bands between them, 1 and 2 of them, and 63, 64, 65 where the frame
    has the bands for it.  On 200 bands the second frame occupies bands 128 and 129 both: a band sum that stops at 128 words
    must then lose survivors that the tiles of band 129 stand behind."""
    nty = -(-roi_h // TH)
    if nty >= 200:
        return [(0, 64, 129, 140, nty - 1), (0, 1, 67, 69, 72, 128, 129, 131, nty - 1)]
    if nty >= 130:
        return [(0, 64, 129), (0, 1, 67, 69, 72, 129)]
    assert nty == 8
    return [(0, 2, 5, 7), (1, 4, 6)]


def empty_bands(roi_w, roi_h, k, seed):
    out = []
    for s, occ in enumerate(occupied_bands(roi_h)):
        cv = Canvas(roi_w, roi_h, k)
        for ty in occ:
            for tx in range(cv.tx):
                cv.ramp_tile(tx, ty)
        out.append((f"o{s}", cv.B))
    return out


def tile_ramp(roi_w, roi_h, k, seed):
    """Tile t holds 1 + (t * 2654435761 % 13) survivors in each of its ramp rows: a tile or a band left out of a sum moves
    every later position."""
    cv = Canvas(roi_w, roi_h, k)
    for ty in range(cv.ty):
        for tx in range(cv.tx):
            cv.ramp_tile(tx, ty)
    return [("ramp", cv.B)]


def render(B, holes, rng):
    """The seed as bytes: `hi` bytes above the floor where B, holes elsewhere."""
    floor = 0 if holes == "zero" else FLOOR_BYTE
    f = rng.integers(floor + 1, 256, size=B.shape).astype(np.uint8)
    if holes == "zero":
        f[~B] = 0
    else:
        lo = rng.integers(0, floor + 1, size=B.shape).astype(np.uint8)
        lo.reshape(-1)[::3] = floor            # the floor byte itself, everywhere among the holes
        f[~B] = lo[~B]
    return f


# --------------------------------------------------------------------------------------------------------------- patterns
class Pattern:
    """The frames of one (generator, shape, k, holes, seed) and, computed once, what the oracle's median leaves of them."""

    def __init__(self, generator, shape, k, holes, seed):
        self.generator, self.shape, self.k, self.holes, self.seed = generator, shape, k, holes, seed
        self.roi_w, self.roi_h = SHAPES[shape]
        self.border, self.dmin, self.scale = BORDER[k], dmin_of(holes), SCALE
        self.w, self.h = self.roi_w + 2 * self.border, self.roi_h + 2 * self.border
        self.tx, self.ty = tiles(self.roi_w, self.roi_h)
        rng = np.random.default_rng([seed, k, HOLES.index(holes)])
        seeds = globals()[generator](self.roi_w, self.roi_h, k, seed)
        self.names = [n for n, _ in seeds]
        self.frames = [render(B, holes, rng) for _, B in seeds]
        self._med = self._valid = self._outside = None

    def __repr__(self):
        return f"{self.generator}-{self.shape}-k{self.k}-{self.holes}"

    @property
    def medians(self):
        if self._med is None:
            self._med = [oracle.median_u8(f, self.k) for f in self.frames]
        return self._med

    def _keep(self, med):
        d = med.astype(np.float32) * np.float32(self.scale)
        return (d > np.float32(self.dmin)) & (med != 0)       # (W = q32 * d with the default Q: zero exactly at d = 0)

    @property
    def valid(self):
        """Per frame: the survivors over the ROI-linear pixel index, from the oracle's median."""
        if self._valid is None:
            b = self.border
            self._valid = [self._keep(m[b:b + self.roi_h, b:b + self.roi_w]).reshape(-1) for m in self.medians]
        return self._valid

    @property
    def outside(self):
        """Per frame: what a count would find over the whole tile grid, the columns and rows beyond the ROI included (the
        border as filtered, the frame's edge repeated beyond it).  Only the model's tail slips look there."""
        if self._outside is None:
            b, gh, gw = self.border, self.ty * TH, self.tx * TW
            self._outside = []
            for m in self.medians:
                v = self._keep(m[b:, b:])[:gh, :gw]
                self._outside.append(np.pad(v, ((0, gh - v.shape[0]), (0, gw - v.shape[1])), mode="edge"))
        return self._outside

    def pix(self):
        v, u = np.mgrid[self.border:self.border + self.roi_h, self.border:self.border + self.roi_w]
        return (v * self.w + u).reshape(-1).astype(np.uint32)


@functools.lru_cache(maxsize=None)
def pattern(generator, shape, k, holes, seed=0):
    return Pattern(generator, shape, k, holes, seed)


def count_table(valid, roi_w, roi_h):
    """-> (tiles_y, 32, tiles_x) survivors per tile row."""
    tx, ty = tiles(roi_w, roi_h)
    g = np.zeros((ty * TH, tx * TW), dtype=bool)
    g[:roi_h, :roi_w] = np.asarray(valid).reshape(roi_h, roi_w)
    return g.reshape(ty, TH, tx, TW).sum(axis=3)


# ------------------------------------------------------------------------------------------------------------------ model
def callback_model(valid, roi_w, roi_h, slip=None, outside=None):
    """The hand-off of k_callback_bs_compact / _pipe restated: row counts of every tile -> the published dwords (two
    9-bit counts and a tag) and the band accumulators -> the bands above -> a row's total over the band -> the part
    left of the tile -> base -> rank inside the 64-column steps.  -> the pixel index stored at every output position
    below the frame's count (-1: nothing stored).  One slip at a time; never the expected answer."""
    assert slip is None or slip in SLIPS, slip
    tx, ty = tiles(roi_w, roi_h)
    gh, gw = ty * TH, tx * TW
    V = np.zeros((gh, gw), dtype=bool)
    V[:roi_h, :roi_w] = np.asarray(valid).reshape(roi_h, roi_w)
    # what the count looks at: the scatter's pixels, unless a clip is missing
    C = V
    if slip in ("tail_cols_counted", "tail_rows_counted", "group_not_clipped"):
        assert outside is not None and outside.shape == (gh, gw)
        C = V.copy()
        if slip == "tail_cols_counted":
            C[:roi_h, roi_w:] = outside[:roi_h, roi_w:]
        elif slip == "tail_rows_counted":
            C[roi_h:, :roi_w] = outside[roi_h:, :roi_w]
        else:                                   # xl < x_end decides for the lane's whole group of 4
            end = min(-(-roi_w // GROUP) * GROUP, gw)
            C[:roi_h, roi_w:end] = outside[:roi_h, roi_w:end]
    cnt = C.reshape(ty, TH, tx, TW).sum(axis=3).astype(np.int64)           # (band, row, tile)
    # publish: dword p of a tile = tag | rows 2p | 2p + 1 << 9; {1, tile total} onto the band's accumulator
    word = (1 << 31) | cnt[:, 0::2, :] | (cnt[:, 1::2, :] << 9)
    band_acc = cnt.sum(axis=(1, 2))
    # look: the fields of every dword of the band
    mask = 0xff if slip == "count_8bit" else 0x1ff
    c0, c1 = word & mask, (word >> 9) & mask
    if slip == "pair_swapped":
        c0, c1 = c1, c0
    read = np.empty_like(cnt)
    read[:, 0::2, :], read[:, 1::2, :] = c0, c1
    if slip == "left_first_16_tiles":
        read[:, :, 16:] = 0
    total = read.sum(axis=2)                                               # a row over the band
    left = np.cumsum(read, axis=2) - (0 if slip == "left_includes_self" else read)
    first = {"above_first_64": 64, "above_first_128": 128}.get(slip, ty)
    above = np.array([band_acc[:min(b, first)].sum() for b in range(ty)], dtype=np.int64)
    rows_above = np.cumsum(total, axis=1) - total
    base = above[:, None, None] + rows_above[:, :, None] + left            # (band, row, tile)
    last = ty - 1
    count = int(above[last] + (0 if slip == "band_total_for_count" else total[last].sum()))
    # scatter: 64 columns per step, the rank carried from step to step
    unit = STEP if slip == "step_rank_restarts" else TW
    Vu = V.reshape(gh, gw // unit, unit)
    rank = (np.cumsum(Vu, axis=2) - Vu).reshape(gh, gw)
    pos = np.repeat(base.reshape(gh, tx), TW, axis=1) + rank
    out = np.full(count, -1, dtype=np.int64)
    ys, xs = np.nonzero(V)
    p = pos[ys, xs]
    keep = p < count
    out[p[keep]] = (ys * roi_w + xs)[keep]
    return out


def killed(valid, roi_w, roi_h, slip, outside):
    return not np.array_equal(callback_model(valid, roi_w, roi_h, slip, outside), np.flatnonzero(valid))
