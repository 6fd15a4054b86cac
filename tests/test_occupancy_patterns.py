"""What the occupancy patterns (tests/occupancy_patterns.py) reach, that the numpy model of the compaction equals
np.flatnonzero(valid) on every one of them, and the kill matrix of its named slips -- at exactly the cases, tile sizes
and seeds tests/test_compact_occupancy_gpu.py runs (its CASES, PATTERN_TESTS and LADDER are imported here).  No GPU."""
import os
import re

import numpy as np
import pytest

import occupancy_patterns as op
import oracle
from route_model import route
from test_compact_occupancy_gpu import CASES, LADDER, PATTERN_TESTS, paths_for

import disparity_to_point_cloud_amd as d2pc

ALL_CASES = [c for tile in (2048, 1024, 4096) for c in CASES[tile]]
IDS = [repr(c) for c in ALL_CASES]
FAMILIES = ("run_counts", "slot_only", "tile_steps", "periods", "row_ends", "ragged_tail")
PATTERN_SLIPS = [s for s in op.SLIPS if s not in op.LADDER_ONLY_SLIPS + op.UNKILLABLE_SLIPS + op.DEVICE_UNREACHABLE_SLIPS]
CU_DEFAULT = 256


def of_family(family, tile=2048):
    return [c for c in CASES[tile] if c.family == family]


# ---------------------------------------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("case", ALL_CASES, ids=IDS)
def test_case_shapes(case):
    """At least four frames per launch, different masks; 66 to 130 tiles (200 for tile_steps, whose N = 128 needs two
    whole empty groups between two full tiles); more than one group, more than two for tile_steps; inside the host's
    size rule."""
    m = case.masks
    assert len(m) >= 4 and len({v.tobytes() for v in m.values()}) >= (1 if case.roi_w == 1 else min(len(m), 3))
    counts = sorted(int(v.sum()) for v in m.values())
    assert counts[0] != counts[-1]                      # frames with very different counts in one launch
    lo, hi = (op.STEP_TILES, op.STEP_TILES) if case.family == "tile_steps" else (66, 130)
    assert lo <= case.tiles <= hi, case.tiles
    assert case.tiles > (2 if case.family == "tile_steps" else 1) * op.GROUP_TILES
    assert (case.h + 4097) * case.w * 4 <= 2**32 - 1


def test_every_generator_runs_at_every_tile_size():
    for tile in (2048, 1024, 4096):
        assert {c.family for c in CASES[tile]} == set(FAMILIES)
        assert len({c.name for c in CASES[tile]}) == len(CASES[tile])


# ----------------------------------------------------------------------------------------------------------------- reach
@pytest.mark.parametrize("tile", [2048, 1024, 4096])
def test_run_counts_reach(tile):
    """Every listed count, in every run position of a tile, in all three placements; `front` / `back` really are."""
    (case,) = of_family("run_counts", tile)
    rpt = tile // op.RUN
    m = case.masks
    for name in ("front", "back", "seeded"):
        c = op.run_count_table(m[name])
        pos = np.arange(len(c)) % rpt
        for want in op.RUN_COUNTS:
            assert set(pos[c == want]) == set(range(rpt)), (name, want)
        assert set(c) == set(op.RUN_COUNTS)
    runs = m["front"][:len(m["front"]) // op.RUN * op.RUN].reshape(-1, op.RUN)
    assert all(r[:r.sum()].all() for r in runs[:64])
    runs = m["back"][:len(m["back"]) // op.RUN * op.RUN].reshape(-1, op.RUN)
    assert all(r[op.RUN - r.sum():].all() for r in runs[:64])
    s = m["seeded"].reshape(-1, op.RUN)
    part = s[(s.sum(axis=1) > 2) & (s.sum(axis=1) < 254)]
    assert not any(r[:r.sum()].all() or r[op.RUN - r.sum():].all() for r in part)   # neither front nor back
    # the in-place pack's premise on the worst layouts: a survivor's rank never exceeds its offset in the run
    for name in m:
        r = m[name][:len(m[name]) // op.RUN * op.RUN].reshape(-1, op.RUN)
        rank = np.cumsum(r, axis=1) - r
        assert np.all(rank[r] <= np.broadcast_to(np.arange(op.RUN), r.shape)[r])
    # the scatter's slot boundary s * 64 >= c: counts on, one below and one above each multiple of 64
    assert {63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256} <= set(op.run_count_table(m["seeded7"]))


def test_slot_only_reach():
    slot, lane, load = of_family("slot_only")
    for k in range(4):
        m = slot.masks[f"slot{k}"].reshape(-1, 4, op.SLOT)
        assert m[:, k].all() and not np.delete(m, k, axis=1).any()
    assert [int(n[4:]) for n in lane.masks if n != "none"] == list(op.LANES)
    for L in op.LANES:
        m = lane.masks[f"lane{L}"].reshape(-1, op.SLOT)
        assert m[:, L].all() and m.sum() == len(m)
    for j in range(4):
        m = load.masks[f"load{j}"].reshape(-1, op.LOAD)
        assert m[:, j].all() and m.sum() == len(m)
    for tile in (1024, 4096):
        assert [c.name for c in of_family("slot_only", tile)] == ["slot_only_slot"]


@pytest.mark.parametrize("tile", [2048, 1024, 4096])
def test_tile_steps_reach(tile):
    """Every N: a full tile, exactly N empty ones, a full tile, with survivors before (a prefix to carry); N = 64 empties
    one whole group, N = 128 two consecutive ones, and the tile after them is a group's first."""
    case = of_family("tile_steps", tile)[0]
    assert case.name == "tile_steps" and list(case.masks) == [f"step{N}" for N in op.STEPS]
    whole = {}
    for N in op.STEPS:
        t = case.masks[f"step{N}"].reshape(-1, tile).sum(axis=1)
        a = op.STEP_START[N]
        assert t[a] == tile and np.all(t[a + 1:a + 1 + N] == 0) and t[a + 1 + N] == tile
        assert np.all(t[:a] > 0) and np.all(t[a + 2 + N:] > 0) and np.all(t[:a] <= 13)
        g = t[:len(t) // op.GROUP_TILES * op.GROUP_TILES].reshape(-1, op.GROUP_TILES).sum(axis=1)
        whole[N] = list(np.flatnonzero(g == 0))
    assert whole[64] == [1] and whole[128] == [1, 2] and whole[127] == [1] and whole[65] == [1]
    assert (op.STEP_START[63] + 64) % op.GROUP_TILES == 0 and (op.STEP_START[64] + 65) % op.GROUP_TILES == 0


def test_tile_singles_reach():
    (case,) = [c for c in CASES[2048] if c.name == "tile_singles"]
    tile, g = case.tile, op.GROUP_TILES * case.tile
    at = {k: np.flatnonzero(v) for k, v in case.masks.items() if k != "all"}
    assert all(len(v) == 1 for v in at.values())
    assert at["tile_first"][0] % tile == 0 and at["tile_last"][0] % tile == tile - 1
    assert at["group_first"][0] % g == 0 and at["group_first"][0] > 0 and at["group_last"][0] % g == g - 1
    assert at["frame_last"][0] == case.roi_n - 1


def test_periods_reach():
    (case,) = of_family("periods")
    assert list(case.masks) == [f"p{p}" for p in op.PERIODS]
    for p in op.PERIODS:
        i = np.flatnonzero(case.masks[f"p{p}"])
        assert np.all(np.diff(i) == p) and i[0] < p
        for unit in (op.LOAD, op.SLOT, op.RUN, op.BATCH, case.tile):   # beats: every residue of the unit that p allows
            assert len(set(i % unit)) == unit // np.gcd(unit, p) or len(i) < unit


def test_row_ends_reach():
    cases = of_family("row_ends")
    assert [c.roi_w for c in cases] == list(op.WIDTHS)
    vec = {c.roi_w: c.roi_w % 4 == 0 and c.border % 4 == 0 for c in cases}
    assert sorted(w for w in vec if vec[w]) == [64, 200, 256] and not vec[255] and not vec[257]   # with and without 16-byte rows
    for c in cases:
        m = c.masks["cols"].reshape(c.roi_h, c.roi_w)
        assert m[:, 0].all() and m[:, -1].all() and m.sum() == c.roi_h * min(c.roi_w, 2)
        r = c.masks["cols_rows"].reshape(c.roi_h, c.roi_w)
        assert r[0].all() and r[-1].all() and (r[1:-1, 1:-1].sum() == 0)
    # either side of the one-wrap shortcut's roi_w >= 256, with survivors that a run reaches after a wrap
    assert {255, 256, 257} <= set(vec)
    assert [c.roi_w for c in of_family("row_ends", 1024)] == [255, 256] == [c.roi_w for c in of_family("row_ends", 4096)]


@pytest.mark.parametrize("tile", [2048, 1024, 4096])
def test_ragged_tail_reach(tile):
    cases = of_family("ragged_tail", tile)
    want = op.tails(tile) if tile == 2048 else (1, 64, tile - 1)
    assert [c.roi_n % tile for c in cases] == list(want)
    for c in cases:
        m = c.masks
        assert m["tail_valid"][-2 * tile:].all() and 0 < m["tail_valid"][:-2 * tile].mean() < 0.25
        assert not m["tail_holes"][-2 * tile:].any() and m["tail_holes"][:-2 * tile].all()
        assert m["last_only"].sum() == 1 and m["last_only"][-1] and m["all"].all()
    assert any(c.roi_w % 4 == 0 and c.border % 4 == 0 for c in cases) and any(c.roi_w % 4 for c in cases)


@pytest.mark.parametrize("case", CASES[2048], ids=[c.name for c in CASES[2048]])
def test_every_case_meets_every_hole_kind_dtype_and_setting(case):
    p = paths_for(case)
    assert {x.kind for x in p} == set(op.HOLE_KINDS)
    assert {x.dtype for x in p} == {"f32", "u8", "u16"} and {x.idx for x in p} == {True, False} and {x.vec for x in p} == {True, False}
    assert {x.algo for x in p} == {0, 1, 2, 3, 4} and {x.batch for x in p} == {"own", "big", "below_big"}
    assert {dict(x.tune).get("resident_pxt") for x in p} >= {32, 64} and sum(x.oracle for x in p) == 1
    for a in (1, 2, 3, 4):   # every algorithm: with and without indices, two hole kinds or more
        mine = [x for x in p if x.algo == a]
        assert {x.idx for x in mine} == {True, False} and len({x.kind for x in mine}) >= 2, a
    assert all(not x.exp for x in p if x.algo != 4 and "onepass_form" not in dict(x.tune))


def test_every_experiment_form_meets_every_generator():
    seen = {}
    for c, p in PATTERN_TESTS:
        f = dict(p.tune).get("onepass_form")
        if f:
            seen.setdefault(f, set()).add(c.family)
    assert set(seen) == {1, 3, 4, 5, 6, 7}
    assert all(v == set(FAMILIES) for v in seen.values()), seen


def test_big_batch_paths_lie_either_side_of_the_rule():
    for c in CASES[2048]:
        n = -(-20480 // c.tiles)
        assert n >= 4 and route(0, c.roi_n, n)[0] == 2 and route(0, c.roi_n, n - 1)[0] in (1, 3)


@pytest.mark.parametrize("kind", op.HOLE_KINDS)
@pytest.mark.parametrize("dtype", ["f32", "u8", "u16"])
def test_frames_hold_holes_of_the_kind_and_nothing_else_invalid(kind, dtype):
    if kind == "nan" and dtype != "f32":
        with pytest.raises(AssertionError):
            op.frames_for([], 8, 8, 0, dtype, kind, 0)
        return
    case = of_family("periods")[0]
    masks = list(case.masks.values())[:2]
    d = op.frames_for(masks, case.h, case.w, case.border, dtype, kind, 5)
    b = case.border
    for m, fr, dec in zip(masks, d.frames, d.decoded):
        roi = dec[b:case.h - b, b:case.w - b].reshape(-1)
        assert np.all(roi[m] > op.FLOOR) and np.all(np.isfinite(roi[m])) and np.all(dec[:b] > op.FLOOR)
        holes = roi[~m]
        if kind == "zero":
            assert np.all(holes == 0)
        elif kind == "nan":
            assert np.all(np.isnan(holes))
        else:
            assert np.all((holes > 0) & (holes <= op.FLOOR)) and (holes == op.FLOOR).any() and d.dmin == op.FLOOR


# ------------------------------------------------------------------------------------------------------------- the model
@pytest.fixture(scope="module")
def matrix():
    """{slip: {case name: number of masks of the case it kills}} for the 2,048-pixel cases, the model without a slip
    checked on the way."""
    out = {s: {} for s in op.SLIPS}
    for c in CASES[2048]:
        for name, m in c.masks.items():
            assert not op.killed(m, c.roi_w, c.tile, None), (c, name)
        for s in op.SLIPS:
            out[s][c.name] = sum(op.killed(m, c.roi_w, c.tile, s) for m in c.masks.values())
    return out


@pytest.mark.parametrize("case", CASES[1024] + CASES[4096], ids=[repr(c) for c in CASES[1024] + CASES[4096]])
def test_model_equals_flatnonzero_at_the_other_tile_sizes(case):
    for name, m in case.masks.items():
        assert not op.killed(m, case.roi_w, case.tile, None), name


def _family_cells(matrix):
    cells = {}
    for s in op.SLIPS:
        for fam in FAMILIES:
            names = [c.name for c in of_family(fam)]
            k = sum(matrix[s][n] > 0 for n in names)
            cells[s, fam] = "X" if k == len(names) else "." if k == 0 else str(k)
    return cells


WANT_MATRIX = """
slip                   run_counts  slot_only   tile_steps  periods     row_ends    ragged_tail
run_tail_dropped       X           1           X           X           X           X
run_full_slot_dropped  X           2           X           .           7           X
rank_not_carried       X           2           X           X           X           X
pack_overwrites        .           .           .           .           .           .
wrap_once_narrow       .           .           .           .           6           8
wrap_once_255          .           .           .           .           .           .
tail_counted           .           .           .           X           X           X
group_first_tile       X           X           X           X           X           X
empty_group_skipped    .           .           1           .           .           .
second_group_trip      .           .           .           .           .           .
scan_unbatched         .           .           .           .           .           .
"""


def render(cells):
    lines = ["slip".ljust(23) + "".join(f.ljust(12) for f in FAMILIES).rstrip()]
    for s in op.SLIPS:
        lines.append((s.ljust(23) + "".join(cells[s, f].ljust(12) for f in FAMILIES)).rstrip())
    return "\n".join(lines)


def test_kill_matrix(matrix):
    """X: the slip changes the model's output for every case of the generator; a digit: for that many of its cases; a dot:
    for none -- asserted too.  Every pattern runs on every algorithm, so a slip with an X or a digit anywhere is killed on
    every algorithm it can occur in.  The matrix is printed in tests/README.md; the two files are held together here."""
    got = render(_family_cells(matrix))
    print("\n" + got)
    assert got == WANT_MATRIX.strip()
    readme = open(os.path.join(os.path.dirname(__file__), "README.md")).read()
    assert WANT_MATRIX.strip() in readme
    for s in PATTERN_SLIPS:
        assert any(v > 0 for v in matrix[s].values()), s
    for s in op.LADDER_ONLY_SLIPS + op.UNKILLABLE_SLIPS + op.DEVICE_UNREACHABLE_SLIPS:
        assert not any(matrix[s].values()), s


def test_pack_order_and_threshold_255_cannot_be_killed(matrix):
    """`pack_overwrites` (slot k + 1 read after slot k's survivors were written): slot k's ranks lie in [c, c + 64) with
    c <= 64 k survivors before it, so its writes end below cell 64 (k + 1) and never reach a cell that is still to be
    read -- "a survivor's rank never exceeds its pixel's offset" makes the order of the four reads free.
    `wrap_once_255` (the one-wrap shortcut from roi_w >= 255 on): a run's pixel lies at most 255 after its first, whose
    column is at most roi_w - 1, so u0 + o <= roi_w + 254 < 2 roi_w for every roi_w >= 255: the shortcut's true bound is
    255, one below the kernel's.  Both shown on every mask of every case, and the second on every (u0, o) at 255."""
    assert not any(matrix["pack_overwrites"].values()) and not any(matrix["wrap_once_255"].values())
    u0, o = np.mgrid[0:255, 0:256]
    assert np.all((u0 + o) // 255 <= 1)
    u0, o = np.mgrid[0:254, 0:256]
    assert np.any((u0 + o) // 254 == 2)        # ... and 254 would be one too far


def test_second_group_trip_is_out_of_a_launch_s_reach():
    """prefix_before's loop over the group words makes a second trip only for a tile of group 65 or later (tile 4,160 on)
    met with known.groups == 0: a block's FIRST tile.  A block of the single pass takes another ticket in every iteration
    in which it holds a tile and leaves only once the frame's tickets are spent, so until then no block retires and only
    co-resident blocks get tiles: first tickets lie below the number of resident blocks, whatever the grid.  The dense
    kernel's static LDS allows four blocks per CU, 1,024 on the device -- a quarter of 4,160.  The slip stays in the
    model (killed there from 4,161 tiles on, asserted with the ladder's masks) and is not claimed for any GPU test."""
    assert op.DEVICE_UNREACHABLE_SLIPS == ("second_group_trip",)
    per_cu = op.LDS_BYTES_PER_CU // op.ONEPASS_LDS_BYTES
    assert per_cu == 4 and per_cu * op.CUS == 1024 < 65 * op.GROUP_TILES
    assert 8 * per_cu * op.CUS < 65 * op.GROUP_TILES * 2     # (not even with half the LDS per block, or twice the CUs)
    assert not any(dict(r.tune).get("onepass_blocks_per_cu") for r in LADDER)   # no rung pretends to


def test_resident_paths_are_served_by_the_resident_blocks():
    """Every compact_algo 3 path of every case -- the router's own shape and resident_pxt 32 / 64 forced -- and the
    default routing of the case's own batch end in the resident blocks on an MI355X (256 CUs); the GPU file asserts
    the same of the device it runs on, so a smaller device fails there instead of passing on the two-pass form."""
    for c, p in PATTERN_TESTS:
        if p.batch == "own" and p.algo in (0, 3):
            t = dict(p.tune)
            assert route(p.algo, c.roi_n, len(c.masks), t.get("pxt_compact", 8), t.get("resident_pxt", 0), cu=CU_DEFAULT)[0] == 3, (c, p.name)
    for c in CASES[2048]:
        for rp in (0, 32, 64):
            assert route(3, c.roi_n, len(c.masks), 8, rp, cu=CU_DEFAULT)[0] == 3, (c, rp)


# ------------------------------------------------------------------------------------------------------------ the ladder
RUNGS = op.ladder_rungs()


def test_ladder_rungs_straddle_the_seams():
    tiles = [r[1] for r in RUNGS]
    for seam in (op.GROUP_TILES, op.SELF_SCAN_TILES, 64 * op.GROUP_TILES, op.SCAN_THREADS * op.SCAN_BATCH):
        assert seam in tiles and seam + 1 in tiles
    # the chunked two-pass reads 512 group totals of 16,384 pixels per trip: 4,096 / 4,097 tiles are 512 / 513 of its groups
    assert 4096 * op.LADDER_TILE == op.CHUNK_TRIP * op.CHUNK_GROUP
    name, t, w, h, n = RUNGS[-1]
    assert n == t * 2048 - 2047 and w * h == n and (h + 4097) * w * 4 <= 2**32 - 1
    assert all((h + 4097) * w * 4 <= 2**32 - 1 and w * h <= 2**28 for _, _, w, h, _ in RUNGS)
    assert max(n for *_, n in RUNGS) * 4 < 68e6      # 16.8 Mpixel: 67 MB of f32 input


def test_ladder_runs_every_algorithm_on_every_rung_and_the_router_turns_at_the_seams():
    for name, tiles, _, _, n in RUNGS:
        mine = [r for r in LADDER if r.rung == name]
        assert {r.algo for r in mine} == {0, 1, 2, 3, 4}
        assert {dict(r.tune).get("resident_pxt", 0) for r in mine if r.algo == 3} == {0, 8, 32, 64}
        for rp, limit in ((8, 1024), (32, 4096), (64, 8192)):
            assert (route(3, n, 1, 8, rp)[0] == 3) == (tiles <= limit)
        assert (route(0, n, 1)[0] == 3) == (tiles <= 8192)
    two = {(r.rung, r.algo) for r in LADDER if r.frames == 2}
    assert two == {("t1025", 1), ("t8193", 1), ("t4097", 2)}


@pytest.mark.parametrize("rung", RUNGS, ids=[r[0] for r in RUNGS])
def test_ladder_masks_and_the_two_ladder_slips(rung):
    """tile_ramp: tile t holds 1 + (t * 2654435761 mod 13) survivors, one full tile per group, whole empty groups before
    the seams; the model equals flatnonzero; `scan_unbatched` is killed exactly from 8,193 tiles on and by no smaller
    rung.  The MODEL also shows `second_group_trip` from 4,161 tiles on (tile 4,160 is the first in group 65), i.e. on the
    8,192 / 8,193 rungs -- but no launch reaches that trip: test_second_group_trip_is_out_of_a_launch_s_reach."""
    name, tiles, w, h, n = rung
    m = op.ladder_mask(name)
    assert m.shape == (n,)
    pad = np.zeros(tiles * 2048, dtype=bool)
    pad[:n] = m
    t = pad.reshape(tiles, 2048).sum(axis=1)
    want = 1 + (np.arange(tiles, dtype=np.uint64) * np.uint64(op.KNUTH) % np.uint64(13)).astype(np.int64)
    groups = -(-tiles // 64)
    full = [g * 64 + (7 * g) % 64 for g in range(groups)]
    empty = op.ramp_empty_groups(tiles)
    assert empty == [g for g in (5, 37, 100) if g < groups - 1] and (tiles < 1024 or 5 in empty)
    assert (tiles < 4096 or 37 in empty) and (tiles < 8192 or 100 in empty)
    for ti in range(tiles):
        if ti // 64 in empty:
            assert t[ti] == 0
        elif ti in full:
            assert t[ti] == (2048 if ti < tiles - 1 or "ragged" not in name else 1)
        elif ti < tiles - 1 or "ragged" not in name:
            assert t[ti] == want[ti]
    assert not op.killed(m, w, 2048, None)
    assert op.killed(m, w, 2048, "second_group_trip") == (tiles >= 4161)
    assert op.killed(m, w, 2048, "scan_unbatched") == (tiles >= 8193)
    assert op.killed(m, w, 2048, "group_first_tile") == (tiles > 64)
    assert op.killed(m, w, 2048, "empty_group_skipped") == bool(empty)


# ----------------------------------------------------------------------------------------------------------- the oracle
@pytest.mark.parametrize("case", CASES[2048], ids=[c.name for c in CASES[2048]])
@pytest.mark.parametrize("dtype,kind", [("f32", "zero"), ("f32", "nan"), ("u8", "floor"), ("u16", "floor")])
def test_oracle_compaction_agrees_with_the_masks(case, dtype, kind):
    """The mask helper against the project's oracle: oracle.reproject_compact of each frame gives pix[valid] and
    valid.sum(), and its points are the unfiltered oracle's at those pixels, bit for bit."""
    masks = list(case.masks.values())
    d = op.frames_for(masks, case.h, case.w, case.border, dtype, kind, 5)
    q = d2pc.make_q()
    pix = op.roi_pixels(case.h, case.w, case.border)
    for m, fr in zip(masks, d.frames):
        wp, wi = oracle.reproject_compact(fr, q, border=case.border, scale=d.scale, min_disparity=d.dmin)
        assert len(wi) == m.sum() and np.array_equal(wi, pix[m])
        full = oracle.reproject(fr, q, border=case.border, scale=d.scale)
        assert np.array_equal(wp.view(np.uint32), full[m].view(np.uint32))


def test_gpu_file_docstring_names_what_was_cut():
    import test_compact_occupancy_gpu as g
    assert re.search(r"CUT:", g.__doc__)
