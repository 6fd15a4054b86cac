"""Built occupancy patterns for ordered compaction (COMPACT): WHERE the survivors lie and HOW MANY tiles a frame has.

A pattern is a boolean mask valid[i] over the ROI-linear pixel index i (row-major inside the ROI: the order of the
reference's loop, cpp:70-76, and the order in which every COMPACT kernel numbers pixels).  `frames_for` writes masks into
frames of a given (h, w, border, dtype): ordinary finite disparities where valid, a hole elsewhere -- 0 (W = 0 for the
default Q), NaN (f32 only) or a value at or below a disparity floor.  The expected answer is plain everywhere:
np.flatnonzero(valid).

`compact_model` restates in numpy the structure the kernels share (runs of 256 pixels -> four wave slots of 64 -> the
scan of a tile's runs -> group / tile prefixes -> position) and applies ONE named slip at a time; it is never the
expected answer.  tests/test_occupancy_patterns.py (no GPU) asserts what each generator reaches and the kill matrix;
tests/test_compact_occupancy_gpu.py runs the patterns through every compaction path.  numpy only."""
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

# structural units (pixels), as parameters of the generators
LANE, LOAD, SLOT, RUN, BATCH = 1, 4, 64, 256, 1024
GROUP_TILES = 64                       # tiles per counting group of the single pass
LEAN_BLOCKS = (8192, 16384)            # lean resident blocks: 32 / 64 pixels per thread
SCAN_THREADS, SCAN_BATCH = 1024, 8     # the two-pass scan: one block per frame, up to 8 tiles per thread in registers
SELF_SCAN_TILES = 1024                 # two-pass frames up to this many tiles: the scatter kernel sums the counts itself
CHUNK_GROUP, CHUNK_TRIP = 16384, 512   # the chunked two-pass: pixels per group, group totals read per trip

RUN_COUNTS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 254, 255, 256)
PLACEMENTS = ("front", "back", "seeded")
LANES = (0, 1, 31, 32, 62, 63)
STEPS = (1, 2, 63, 64, 65, 127, 128)
# first full tile of "full, N empty, full": N = 64 empties exactly group 1, N = 128 groups 1 and 2; N = 63 / 127 end on a
# group's last tile, N = 1 / 2 / 65 straddle a group seam
STEP_START = {1: 62, 2: 62, 63: 0, 64: 63, 65: 62, 127: 0, 128: 63}
STEP_TILES = 200                       # tiles of a tile_steps frame (the second full tile of N = 128 is tile 192)
PERIODS = (3, 5, 63, 65, 255, 257, 2047, 2049)
WIDTHS = (1, 3, 63, 64, 65, 200, 255, 256, 257, 2049)
HOLE_KINDS = ("zero", "nan", "floor")
FLOOR = 8.0                            # the disparity floor of hole kind "floor"
SCALES = {"f32": 1.0, "u8": 0.125, "u16": 1.0 / 64}
KNUTH = 2654435761

SLIPS = ("run_tail_dropped", "run_full_slot_dropped", "rank_not_carried", "pack_overwrites", "wrap_once_narrow",
         "wrap_once_255", "tail_counted", "group_first_tile", "empty_group_skipped", "second_group_trip", "scan_unbatched")
LADDER_ONLY_SLIPS = ("scan_unbatched",)
# no input can show these two (tests/test_occupancy_patterns.py proves it on every mask and says why)
UNKILLABLE_SLIPS = ("pack_overwrites", "wrap_once_255")
# The model shows `second_group_trip` on masks of 4,161 tiles and more, but no launch can reach it.  prefix_before's loop
# over the group words (64 at a time) makes a second trip only for a tile of group 65 or later (tile 4,160 on) met with
# known.groups == 0, i.e. as a block's FIRST tile: later tiles start from the groups the block already knows.  A block of
# the single pass that holds a tile takes another ticket every iteration and leaves only once the frame's tickets are
# spent, so no block retires before that and only the co-resident blocks ever get a tile: first tickets lie below the
# number of resident blocks -- at about 38.5 KiB of LDS per block (ONEPASS_LDS_BYTES) and 160 KiB per CU, 4 per CU, 1,024 on
# 256 CUs -- whatever the grid.  The slip is model-only, like the two above.
DEVICE_UNREACHABLE_SLIPS = ("second_group_trip",)
ONEPASS_LDS_BYTES = 4 * 8 * 256 * 4 + 3 * 8 * 256 + 600   # s_tile (four tiles of raw pixels), s_off, the small arrays
LDS_BYTES_PER_CU, CUS = 160 * 1024, 256


def tails(tile):
    return (1, 3, 63, 64, 65, 255, 256, 257, tile - 1)


# ------------------------------------------------------------------------------------------------------------ generators
def run_counts(roi_n, tile, seed):
    """Four masks.  Run r of 256 pixels holds RUN_COUNTS[(r + shift) % 15] survivors -- at the run's front, at its
    back, at seeded positions, and (fourth mask, shift 7) at seeded positions again.  15 is coprime to the runs of a
    tile (4, 8 or 16), so every count meets every run position of a tile."""
    rng = np.random.default_rng(seed)
    runs = -(-roi_n // RUN)
    out = {}
    for name, place, shift in (("front", "front", 0), ("back", "back", 0), ("seeded", "seeded", 0), ("seeded7", "seeded", 7)):
        c = np.array(RUN_COUNTS)[(np.arange(runs) + shift) % len(RUN_COUNTS)]
        if place == "front":
            m = np.arange(RUN)[None, :] < c[:, None]
        elif place == "back":
            m = np.arange(RUN)[None, :] >= RUN - c[:, None]
        else:
            order = np.argsort(rng.random((runs, RUN)), axis=1)      # a seeded permutation per run
            m = order < c[:, None]
        out[name] = m.reshape(-1)[:roi_n].copy()
    return out


def run_count_table(mask):
    """Survivors of every whole run of a mask."""
    n = len(mask) // RUN
    return mask[:n * RUN].reshape(n, RUN).sum(axis=1)


def slot_only(roi_n, which):
    """Survivors only in slot k of every run ("slot"), only in one lane column ("lane"), only in one pixel of each
    4-pixel load ("load")."""
    i = np.arange(roi_n)
    if which == "slot":
        out = {f"slot{k}": (i % RUN) // SLOT == k for k in range(4)}
    elif which == "lane":
        out = {f"lane{L}": i % SLOT == L for L in LANES}
    else:
        out = {f"load{j}": i % LOAD == j for j in range(4)}
    out["none"] = np.zeros(roi_n, dtype=bool)      # (a frame without a survivor beside them: very different counts in one launch)
    return out


def sparse_tiles(tiles, tile, seed):
    """(tiles, tile) mask: tile t holds 1 + (t * 2654435761 mod 13) survivors at seeded, distinct positions."""
    rng = np.random.default_rng(seed)
    n = 1 + (np.arange(tiles, dtype=np.uint64) * np.uint64(KNUTH) % np.uint64(13)).astype(np.int64)
    start = rng.integers(0, tile, size=tiles)
    m = np.zeros((tiles, tile), dtype=bool)
    for j in range(13):   # 157 j is distinct modulo any power of two above 13 * 157 ... and modulo 1,024 too (157 is odd)
        rows = np.flatnonzero(n > j)
        m[rows, (start[rows] + 157 * j) % tile] = True
    return m


def tile_steps(roi_n, tile, seed):
    """One mask per N of STEPS: tile STEP_START[N] full, the next N tiles empty, the next full; every other tile sparse
    (sparse_tiles), so that a prefix is carried into and across the empty stretch."""
    tiles = -(-roi_n // tile)
    assert tiles >= STEP_TILES
    out = {}
    for N in STEPS:
        m = sparse_tiles(tiles, tile, seed + N)
        a = STEP_START[N]
        m[a] = True
        m[a + 1:a + 1 + N] = False
        m[a + 1 + N] = True
        out[f"step{N}"] = m.reshape(-1)[:roi_n].copy()
    return out


def tile_singles(roi_n, tile):
    """A single survivor: on the first / last pixel of a tile (65), on the first / last pixel of a group (1), on the
    last pixel of the frame."""
    g = GROUP_TILES * tile
    at = {"tile_first": 65 * tile, "tile_last": 66 * tile - 1, "group_first": g, "group_last": 2 * g - 1, "frame_last": roi_n - 1}
    out = {}
    for k, i in at.items():
        assert 0 <= i < roi_n
        m = np.zeros(roi_n, dtype=bool)
        m[i] = True
        out[k] = m
    out["all"] = np.ones(roi_n, dtype=bool)        # (a full frame beside them: very different counts in one launch)
    return out


def periods(roi_n, seed):
    rng = np.random.default_rng(seed)
    i = np.arange(roi_n)
    return {f"p{p}": i % p == int(rng.integers(0, p)) for p in PERIODS}


def row_ends(roi_w, roi_h):
    """Survivors only in the first and last ROI column; with the whole first and last ROI rows added; each column alone;
    the two rows alone."""
    v, u = np.divmod(np.arange(roi_w * roi_h), roi_w)
    cols = (u == 0) | (u == roi_w - 1)
    return {"cols": cols, "cols_rows": cols | (v == 0) | (v == roi_h - 1), "first_col": u == 0, "last_col": u == roi_w - 1,
            "rows": (v == 0) | (v == roi_h - 1)}


def ragged_tail(roi_n, tile):
    """tail_valid: the frame's last 2 tile pixels all valid (a clamped tail load that counted would add survivors), one
    pixel in five before; tail_holes: the mirror image; last_only; all."""
    i = np.arange(roi_n)
    tail = i >= roi_n - 2 * tile
    return {"tail_valid": tail | (i % 5 == 0), "tail_holes": ~tail, "last_only": i == roi_n - 1, "all": np.ones(roi_n, dtype=bool)}


def tile_ramp(tiles, tile, seed, roi_n=None):
    """The ladder's occupancy: sparse_tiles, one wholly full tile in every group (tile 64 g + 7 g mod 64), and wholly
    empty groups 5, 37 and 100 where the frame has them before its last group: every tile's prefix differs from its
    neighbours', and a dropped or doubled group moves every later point."""
    m = sparse_tiles(tiles, tile, seed)
    groups = -(-tiles // GROUP_TILES)
    for g in range(groups):
        t = g * GROUP_TILES + (7 * g) % GROUP_TILES
        if t < tiles:
            m[t] = True
    for g in ramp_empty_groups(tiles):
        m[g * GROUP_TILES:(g + 1) * GROUP_TILES] = False
    m = m.reshape(-1)
    return m if roi_n is None else m[:roi_n].copy()


def ramp_empty_groups(tiles):
    return [g for g in (5, 37, 100) if (g + 2) * GROUP_TILES <= tiles]


# ----------------------------------------------------------------------------------------------------------------- frames
def frames_for(masks, h, w, border, dtype, kind, seed):
    """-> SimpleNamespace(frames, dmin, scale, decoded): one (h, w) frame per mask.  Valid ROI pixels and everything
    outside the ROI hold ordinary finite disparities above FLOOR; holes hold 0, NaN, or (kind "floor", to be run with
    min_disparity = FLOOR) values in (0, FLOOR] with FLOOR itself among them."""
    assert kind in HOLE_KINDS and dtype in SCALES and not (kind == "nan" and dtype != "f32")
    rng = np.random.default_rng(seed)
    rh, rw = h - 2 * border, w - 2 * border
    scale = SCALES[dtype]
    frames = []
    for m in masks:
        assert m.shape == (rh * rw,) and m.dtype == bool
        if dtype == "f32":
            fr = (rng.integers(72, 960, size=(h, w)) / 8.0).astype(np.float32)          # 9.0 .. 119.875
            hole = {"zero": lambda n: np.zeros(n), "nan": lambda n: np.full(n, np.nan),
                    "floor": lambda n: rng.integers(1, 65, size=n) / 8.0}[kind]
        elif dtype == "u8":
            fr = rng.integers(70, 256, size=(h, w)).astype(np.uint8)                   # 8.75 .. 31.875
            hole = {"zero": lambda n: np.zeros(n), "floor": lambda n: rng.integers(1, 65, size=n)}[kind]
        else:
            fr = rng.integers(600, 65536, size=(h, w)).astype(np.uint16)               # 9.375 .. 1023.98
            hole = {"zero": lambda n: np.zeros(n), "floor": lambda n: rng.integers(1, 513, size=n)}[kind]
        roi = fr[border:h - border, border:w - border]
        holes = ~m.reshape(rh, rw)
        vals = hole(int(holes.sum())).astype(fr.dtype)
        if kind == "floor" and len(vals):
            vals[0] = {"f32": FLOOR, "u8": 64, "u16": 512}[dtype]                      # the floor itself: d <= floor is a hole
        roi[holes] = vals
        frames.append(fr)
    decoded = [f.astype(np.float32) * np.float32(scale) for f in frames]
    return SimpleNamespace(frames=frames, dmin=FLOOR if kind == "floor" else -np.inf, scale=scale, decoded=decoded)


def roi_pixels(h, w, border):
    """Image-linear index of every ROI pixel, in ROI order."""
    v, u = np.mgrid[border:h - border, border:w - border]
    return (v * w + u).reshape(-1).astype(np.uint32)


# ------------------------------------------------------------------------------------------------------------------ cases
def _factor(n, prefer4):
    """roi_w x roi_h = n with 60 <= roi_w <= 4100, a multiple of four if there is one and it is asked for."""
    cands = [w for w in range(60, 4101) if n % w == 0]
    by4 = [w for w in cands if w % 4 == 0]
    if prefer4 and by4:
        return by4[0]
    return cands[0] if cands else None


def ragged_shape(t, tile):
    """The first k in 66.. for which k tile + t has a usable factorisation -> (roi_w, roi_h)."""
    for k in range(66, 131):
        n = k * tile + t
        w = _factor(n, prefer4=True)
        if w:
            return w, n // w
    raise AssertionError((t, tile))


class Case:
    """One launch's worth of masks on one frame shape and one tile size."""

    def __init__(self, name, family, tile, roi_w, roi_h, border, build):
        self.name, self.family, self.tile, self.roi_w, self.roi_h, self.border = name, family, tile, roi_w, roi_h, border
        self.h, self.w, self.roi_n = roi_h + 2 * border, roi_w + 2 * border, roi_w * roi_h
        self.tiles = -(-self.roi_n // tile)
        self._build = build

    @property
    def masks(self):
        return _masks(self)

    def __repr__(self):
        return f"{self.name}@{self.tile}"


@lru_cache(maxsize=4)
def _masks(case):
    m = case._build(case)
    assert len(m) >= 4 and all(v.shape == (case.roi_n,) for v in m.values())
    return m


def make_cases(tile, thin=False):
    """The cases of one tile size.  thin (the tile sizes of the experiment build): one or two cases per generator."""
    cases = []

    def add(name, family, roi_w, roi_h, border, build):
        cases.append(Case(name, family, tile, roi_w, roi_h, border, build))

    rows70 = 70 * tile // 512
    add("run_counts", "run_counts", 512, rows70, 4, lambda c: run_counts(c.roi_n, c.tile, 11))
    for which in ("slot", "lane", "load")[:1 if thin else 3]:
        add(f"slot_only_{which}", "slot_only", 512, rows70, 3, lambda c, which=which: slot_only(c.roi_n, which))
    rows200 = STEP_TILES * tile // 512
    add("tile_steps", "tile_steps", 512, rows200, 0, lambda c: tile_steps(c.roi_n, c.tile, 23))
    if not thin:
        add("tile_singles", "tile_steps", 512, rows200, 4, lambda c: tile_singles(c.roi_n, c.tile))
    add("periods", "periods", 520, -(-70 * tile // 520) + 1, 4, lambda c: periods(c.roi_n, 37))
    for rw in (WIDTHS if not thin else (255, 256)):
        rh = -(-66 * tile // rw) + 1
        add(f"row_ends_{rw}", "row_ends", rw, rh, 4 if rw % 4 == 0 else 1, lambda c: row_ends(c.roi_w, c.roi_h))
    for t in (tails(tile) if not thin else (1, 64, tile - 1)):
        rw, rh = ragged_shape(t, tile)
        add(f"ragged_tail_{t}", "ragged_tail", rw, rh, 4 if rw % 4 == 0 else 3, lambda c: ragged_tail(c.roi_n, c.tile))
    return cases


# ------------------------------------------------------------------------------------------------------------ the ladder
LADDER_TILE = 2048
LADDER_TILES = (64, 65, 1024, 1025, 4096, 4097, 8192, 8193)
LADDER_RAGGED = (8193, 257, 65281)      # 8193 * 2048 - 2047 = 2^24 + 1 = 257 * 65281


def ladder_rungs():
    """-> [(name, tiles, roi_w, roi_h, roi_n)]: a ROI 2,048 wide by `tiles` rows, and the ragged rung."""
    r = [(f"t{t}", t, LADDER_TILE, t, t * LADDER_TILE) for t in LADDER_TILES]
    t, w, h = LADDER_RAGGED
    assert w * h == t * LADDER_TILE - (LADDER_TILE - 1)
    return r + [(f"t{t}_ragged", t, w, h, w * h)]


@lru_cache(maxsize=2)
def ladder_mask(name):
    for n, tiles, _, _, roi_n in ladder_rungs():
        if n == name:
            return tile_ramp(tiles, LADDER_TILE, 1000 + tiles, roi_n)
    raise KeyError(name)


# -------------------------------------------------------------------------------------------------------------- the model
def compact_model(valid, roi_w, tile, slip=None):
    """-> (count, u, v): the frame's count and, per output position, the ROI column and row of the pixel stored there
    (-1: never written; -2: written from a cell of the run's slice that the pack never filled).  The structure of the
    dense single pass (d2pc_onepass.hip), whose tile / group prefixes the other algorithms share in their own words:

      run (256 pixels) -> four slots of 64 lanes; slot k's ranks start at the survivors of slots 0..k-1; the survivors'
      offsets are packed to the front of the run's slice in place; the scatter phase writes ceil(c / 64) slots of it,
      finding a survivor's column and row from the run's first pixel with at most one wrap if roi_w >= 256 and by
      division otherwise; a run's position in its tile is the sum of the runs before it; a tile's prefix is the sum
      of the complete groups (64 tiles) before its own plus the tiles before it in its own group.

    slip: one of SLIPS.  `scan_unbatched` replaces the prefixes by those of the two-pass scan (1,024 threads, each
    owning ceil(tiles / 1024) consecutive tiles) with the slip in its branch for more than 8 tiles per thread."""
    assert slip is None or slip in SLIPS
    valid = np.asarray(valid, dtype=bool)
    roi_n = len(valid)
    tiles = -(-roi_n // tile)
    ok = np.zeros(tiles * tile, dtype=bool)
    ok[:roi_n] = valid
    if slip == "tail_counted":
        ok[roi_n:] = valid[roi_n - 1]          # the clamped loads repeat the frame's last pixel
    R = tiles * tile // RUN
    ok = ok.reshape(R, RUN)
    rows = np.arange(R)[:, None]
    # count phase: in-place pack of each run's slice (cell j first holds pixel j of the run)
    cells = np.tile(np.arange(RUN), (R, 1))
    src = cells if slip == "pack_overwrites" else cells.copy()     # (the slip reads slot k + 1 after slot k was written)
    filled = np.zeros((R, RUN), dtype=bool)
    c = np.zeros(R, dtype=np.int64)
    prev = np.zeros(R, dtype=np.int64)
    for k in range(4):
        cur = src[:, k * SLOT:(k + 1) * SLOT].copy()
        okk = np.take_along_axis(ok, cur, axis=1)
        base = prev if (slip == "rank_not_carried" and k) else c
        rank = base[:, None] + np.cumsum(okk, axis=1) - okk
        rr = np.broadcast_to(rows, okk.shape)[okk]
        cells[rr, rank[okk]] = cur[okk]
        filled[rr, rank[okk]] = True
        prev = okk.sum(axis=1)
        c = c + prev
    # scatter phase: how many cells of each run are written out
    slots = -(-c // SLOT)
    if slip == "run_tail_dropped":
        slots = c // SLOT
    if slip == "run_full_slot_dropped":
        slots = slots - ((c % SLOT == 0) & (c > 0))
    lim = np.minimum(c, slots * SLOT)
    # positions
    rpt = tile // RUN
    ct = c.reshape(tiles, rpt)
    run_off = (np.cumsum(ct, axis=1) - ct).reshape(-1)
    tile_tot = ct.sum(axis=1)
    t = np.arange(tiles)
    grp = t // GROUP_TILES
    excl = np.cumsum(tile_tot) - tile_tot
    gfirst = excl[grp * GROUP_TILES]          # == the sum of the complete groups before grp
    in_group = excl - gfirst
    gt = np.add.reduceat(tile_tot, np.arange(0, tiles, GROUP_TILES))  # group totals (the last may be partial: never read)
    gcum = np.concatenate([[0], np.cumsum(gt)])
    gsum = gcum[grp]
    if slip == "group_first_tile":
        first = (t % GROUP_TILES == 0) & (grp > 0)
        gsum = gsum - np.where(first, gt[np.maximum(grp - 1, 0)], 0)
    if slip == "empty_group_skipped":
        empty = np.flatnonzero(gt[:-1] == 0) if len(gt) > 1 else np.array([], dtype=int)
        if len(empty):
            gsum = gcum[np.minimum(grp, empty[0])]
    if slip == "second_group_trip":
        gsum = gcum[np.minimum(grp, 64)]
    prefix = gsum + in_group
    count = int(tile_tot.sum())
    if slip == "scan_unbatched":
        per = -(-tiles // SCAN_THREADS)
        owner = t // per
        mine = np.zeros(SCAN_THREADS, dtype=np.int64)
        counted = tile_tot if per <= SCAN_BATCH else np.where(t % per < SCAN_BATCH, tile_tot, 0)
        np.add.at(mine, owner, counted)
        before = np.cumsum(mine) - mine
        prefix = before[owner] + (excl - excl[owner * per])
        count = int(mine.sum())
    pos0 = np.repeat(prefix, rpt) + run_off
    j = np.arange(RUN)[None, :]
    write = j < lim[:, None]
    pos = (pos0[:, None] + j)[write]
    o = cells[write]
    fresh = filled[write]
    run_base = (np.arange(R) * RUN)[:, None] + np.zeros((1, RUN), dtype=np.int64)
    rb = run_base[write]
    wide = roi_w >= (255 if slip == "wrap_once_255" else 256) or slip == "wrap_once_narrow"
    if wide:
        v0, u0 = np.divmod(rb, roi_w)
        uu, vv = u0 + o, v0
        wrap = uu >= roi_w
        uu, vv = np.where(wrap, uu - roi_w, uu), np.where(wrap, vv + 1, vv)
    else:
        vv, uu = np.divmod(rb + o, roi_w)
    uu, vv = np.where(fresh, uu, -2), np.where(fresh, vv, -2)
    inb = pos < roi_n                          # the kernels' guard: a wrong prefix never becomes an out-of-bounds store
    u = np.full(roi_n, -1, dtype=np.int64)
    v = np.full(roi_n, -1, dtype=np.int64)
    u[pos[inb]], v[pos[inb]] = uu[inb], vv[inb]
    return count, u, v


def expected(valid, roi_w):
    """What every algorithm must give, in the model's terms: np.flatnonzero(valid) in ROI order."""
    i = np.flatnonzero(valid)
    u = np.full(len(valid), -1, dtype=np.int64)
    v = np.full(len(valid), -1, dtype=np.int64)
    v[:len(i)], u[:len(i)] = np.divmod(i, roi_w)
    return len(i), u, v


def killed(valid, roi_w, tile, slip):
    cnt, u, v = compact_model(valid, roi_w, tile, slip)
    wc, wu, wv = expected(valid, roi_w)
    return not (cnt == wc and np.array_equal(u, wu) and np.array_equal(v, wv))
