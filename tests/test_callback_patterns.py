"""What the callback patterns (tests/callback_patterns.py) reach on the oracle's median, that the numpy model of the fused
COMPACT kernels' hand-off equals np.flatnonzero(valid) on every one of them, and the kill matrix of its named slips --
at exactly the cases, shapes, window sizes, hole kinds and seeds tests/test_callback_compact_occupancy_gpu.py runs (its
CASES are imported here; a pattern no case of it uses is refused).  No GPU."""
import hashlib

import numpy as np
import pytest

import callback_patterns as cp
import oracle
from test_callback_compact_occupancy_gpu import (BAND_129, CASES, GENERATORS_ON, ROUTINGS, SLIVER_SCALES, SMALL3_EDGE_PARTS, STEADY,
                                                 assert_early_look_meets_band_129, assert_steady, case_id, frame_order, pattern_of,
                                                 route)

import disparity_to_point_cloud_amd as d2pc

KEYS = sorted({(c.generator, ROUTINGS[c.routing][0], c.k, c.holes) for c in CASES})
IDS = ["-".join(map(str, k)) for k in KEYS]


def pat(generator, shape, k, holes):
    """Only the patterns the GPU file runs."""
    assert (generator, shape, k, holes) in KEYS, "no case of the GPU file runs this pattern"
    return cp.pattern(generator, shape, k, holes)


def of(generator):
    return [key for key in KEYS if key[0] == generator]


def table(p, i):
    return cp.count_table(p.valid[i], p.roi_w, p.roi_h)


# ------------------------------------------------------------------------------------------------------ cases and routing
def test_case_list_is_the_issue_s():
    """Every generator on `five`; the ramp and the empty bands on the tall shapes; ramp and tile steps either side of
    16 tiles across; row counts and edges on the odd height and on the one-tile-per-block batch; both window sizes, the
    stereo and the general kernel, and both kinds of hole for every (routing, generator, k); one sliver-scale case."""
    assert len({case_id(c) for c in CASES}) == len(CASES)
    assert set(GENERATORS_ON["five"]) == set(cp.GENERATORS)
    for routing, gens in GENERATORS_ON.items():
        for g in gens:
            for k in (3, 11):
                mine = [c for c in CASES if (c.routing, c.generator, c.k) == (routing, g, k) and c.scale == cp.SCALE]
                assert {c.general_q for c in mine} == {0, 1} and {c.holes for c in mine} == set(cp.HOLES), (routing, g, k)
    assert {"tile_ramp", "empty_bands"} <= set(GENERATORS_ON["tall"]) and set(GENERATORS_ON["tall"]) == set(GENERATORS_ON["tall2"])
    assert all(set(GENERATORS_ON[r]) == set(GENERATORS_ON["tall"]) for r in BAND_129)
    assert {"tile_ramp", "tile_steps"} <= set(GENERATORS_ON["sixteen"]) and set(GENERATORS_ON["sixteen"]) == set(GENERATORS_ON["seventeen"])
    assert {"row_counts", "edges"} <= set(GENERATORS_ON["small3"]) and {"row_counts", "edges"} <= set(GENERATORS_ON["five_odd"])
    sliver = [c for c in CASES if c.scale != cp.SCALE]
    assert [c.scale for c in sliver] == list(SLIVER_SCALES) and SLIVER_SCALES[0] == 1.3e-41
    assert all(c.routing == "five" and c.general_q == 0 and c.holes == "zero" for c in sliver)
    assert sorted(x for part in SMALL3_EDGE_PARTS for x in set(part)) == sorted(cp.EDGE_FRAMES + ("none", "full"))
    for c in CASES:       # a frame without a survivor beside a full one
        if c.generator == "edges":
            names = [pattern_of(c).names[i] for i in frame_order(c, route(c.routing).n)]
            if c.part in (None, 1, 2):
                assert any({names[i], names[i + 1]} == {"none", "full"} for i in range(len(names) - 1)), case_id(c)


def test_router_restated_on_256_cus():
    want = {"five": (16, 16, 5, 8), "five_odd": (16, 16, 5, 8), "five_min": (42, 6, 5, 8), "sixteen": (8, 32, 16, 3),
            "seventeen": (8, 32, 17, 3), "tall": (8, 32, 1, 130), "tall2": (8, 32, 2, 130), "taller": (8, 32, 1, 200),
            "taller2": (8, 32, 2, 200), "small3": (3, 39, 3, 13)}
    for routing, w in want.items():
        r = route(routing)
        assert (r.n, r.per_frame, r.tiles_x, r.tiles_y) == w, (routing, r)
    assert route("five_min").per_frame == route("five_min").tiles_x + 1
    for c in CASES:      # 0.2 to 11 Mpixel of ROI per batch; 13.2 on the two shapes that put band 129 well before a frame's end
        r, p = route(c.routing), pattern_of(c)
        assert 0.2e6 <= r.n * p.roi_w * p.roi_h <= (13.2e6 if c.routing in BAND_129 else 11e6), case_id(c)


@pytest.mark.parametrize("cu", [256, 304, 228, 128])
def test_steady_state_cases_have_fewer_blocks_than_tiles(cu):
    """The frame count follows the CU count: on every device size tried, a steady-state case has one sub-batch, more
    blocks per frame than a band has tiles and fewer than the frame has tiles; small3 keeps one block per tile."""
    for routing in STEADY:
        assert_steady(route(routing, cu), routing)
    r = route("small3", cu)
    assert r.per_frame == r.tpf and r.sub_batches == 1 and r.pipelined
    for c in CASES:      # the frames of every pattern all appear in its batch
        p, n = pattern_of(c), route(c.routing, cu).n
        assert c.part is not None or set(frame_order(c, n)) == set(range(len(p.frames))), case_id(c)


@pytest.mark.parametrize("cu", [256, 304, 228, 128])
def test_which_shapes_ask_the_early_look_for_a_tile_below_more_than_128_bands(cu):
    """A tile takes the early look only if its block draws another tile's ticket while filtering it.  On `tall` the only tile
    with more than 128 bands above is the frame's LAST ticket and on `tall2` the last two: never `prev` beside a valid `cur`
    (tall) or only by an accident of dispatch (tall2).  `taller` / `taller2` keep band 129 more than 2 * per_frame tickets
    before the end."""
    for routing in BAND_129:
        assert_early_look_meets_band_129(route(routing, cu), routing)
    for routing in ("tall", "tall2"):
        r = route(routing, cu)
        assert 129 * r.tiles_x >= r.tpf - 2 and r.tiles_y == 130
        with pytest.raises(AssertionError):
            assert_early_look_meets_band_129(r, routing)


@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_shapes_and_bytes(key):
    p = pat(*key)
    assert (p.w, p.h) == (p.roi_w + 2 * p.border, p.roi_h + 2 * p.border) and p.border >= p.k // 2
    floor = 0 if p.holes == "zero" else cp.FLOOR_BYTE
    for f in p.frames:
        assert f.dtype == np.uint8 and f.shape == (p.h, p.w)
        low = f[f <= floor]
        if p.holes == "floor" and low.size:
            assert (low == floor).any() and (low < floor).any() and low.min() == 0     # the floor byte itself among the holes
    assert np.float32(cp.FLOOR_BYTE) * np.float32(cp.SCALE) == np.float32(cp.dmin_of("floor"))


# ------------------------------------------------------------------------------------------------------------------- reach
@pytest.mark.parametrize("key", of("row_counts"), ids=lambda k: "-".join(map(str, k)))
def test_row_counts_reach(key):
    """Every listed count of a (tile, row) on an even and on an odd tile row, in each frame; every listed row pair."""
    p = pat(*key)
    for i in range(len(p.frames)):
        c = table(p, i)
        even, odd = c[:, 0::2, :], c[:, 1::2, :]
        for want in (cp.FINE_COUNTS if p.k == 3 else cp.COARSE_COUNTS):
            assert (even == want).any() and (odd == want).any(), (key, i, want)
        pairs = set(zip(even.reshape(-1).tolist(), odd.reshape(-1).tolist()))
        assert set(cp.ROW_PAIRS) <= pairs, (key, i, set(cp.ROW_PAIRS) - pairs)
    assert {0, 1, 64, 128, 255, 256} <= set(cp.COARSE_COUNTS) <= set(cp.FINE_COUNTS)
    assert not np.array_equal(p.valid[0], p.valid[1])


@pytest.mark.parametrize("key", of("step_only"), ids=lambda k: "-".join(map(str, k)))
def test_step_only_reach(key):
    p = pat(*key)
    for i in range(len(p.frames)):
        g = p.valid[i].reshape(p.roi_h, p.roi_w)
        tx = int(p.names[i][1:])
        assert not np.delete(g, np.s_[cp.TW * tx:cp.TW * tx + cp.TW], axis=1).any()
        rows = g[:, cp.TW * tx:cp.TW * tx + cp.TW]
        rows = rows[rows.any(axis=1)]
        steps = rows.reshape(len(rows), 4, cp.STEP).sum(axis=2)
        for q in range(4):      # one step full, the other three empty
            assert any(s[q] == cp.STEP and s.sum() == cp.STEP for s in steps), (key, q)
        alone = [int(np.flatnonzero(r)[0]) for r in rows if r.sum() == 1]
        assert {x % cp.STEP for x in alone} >= {0, cp.STEP - 1} and {x % cp.GROUP for x in alone} == set(range(cp.GROUP))
        assert sorted(alone) == sorted(cp.STEP_ONLY_SINGLES)
        assert {y % 2 for y in np.flatnonzero(g.any(axis=1))} == {0, 1}


@pytest.mark.parametrize("key", of("edges"), ids=lambda k: "-".join(map(str, k)))
def test_edges_reach(key):
    p = pat(*key)
    v = {n: p.valid[i].reshape(p.roi_h, p.roi_w) for i, n in enumerate(p.names)}
    assert tuple(p.names) == cp.EDGE_FRAMES
    ys, xs = np.nonzero(v["cols"])
    assert len(set(ys)) == len(ys) and sorted(xs) == cp.edge_columns(p.roi_w)       # each the only one of its row
    full = p.roi_w // cp.TW
    assert {0, cp.TW - 1, cp.TW, cp.TW * full - 1, p.roi_w - 1} == set(xs) and (p.roi_w - 1) % cp.TW != cp.TW - 1
    assert v["first_row"][0].sum() > 3 * 17 and not v["first_row"][1:].any()
    assert v["last_row"][-1].sum() > 3 * 17 and not v["last_row"][:-1].any()
    assert np.flatnonzero(v["first_px"]).tolist() == [0]
    assert np.flatnonzero(v["last_px"]).tolist() == [p.roi_w * p.roi_h - 1]
    assert not v["none"].any() and v["full"].all()


@pytest.mark.parametrize("key", of("tile_steps"), ids=lambda k: "-".join(map(str, k)))
def test_tile_steps_reach(key):
    """Inside a band: a tile with every pixel, exactly N tiles without one, a tile with every pixel; N = 1, 3 on five
    tiles across (3 ends on the ragged tile), N = 1, 3, 4, 5 on sixteen and seventeen."""
    p = pat(*key)
    plans = cp.step_plan(p.roi_w, p.roi_h)
    assert len(plans) == len(p.frames)
    for i, plan in enumerate(plans):
        c = table(p, i)
        t = c.sum(axis=1)                      # (band, tile)
        rows = np.minimum(cp.TH, p.roi_h - cp.TH * np.arange(p.ty))
        width = np.minimum(cp.TW, p.roi_w - cp.TW * np.arange(p.tx))
        for band, chains in plan.items():
            for a, n in chains:
                for e in (a, a + n + 1):
                    assert t[band, e] == rows[band] * width[e] and (c[band, :rows[band], e] == width[e]).all(), (key, band, e)
                assert (t[band, a + 1:a + n + 1] == 0).all(), (key, band, a)
            chained = {x for a, n in chains for x in range(a, a + n + 2)}
            assert all(t[band, x] > 0 for x in range(p.tx) if x not in chained)
        assert {n for ch in plan.values() for _, n in ch} == ({1, 3} if p.tx == 5 else {1, 3, 4, 5})
        assert len(set(plan) | {b + 1 for b in plan}) == 2 * len(plan)      # chains in bands that are no neighbours
    if p.tx == 17:
        assert any(a + n + 1 == 16 for plan in plans for ch in plan.values() for a, n in ch)


@pytest.mark.parametrize("key", of("empty_bands"), ids=lambda k: "-".join(map(str, k)))
def test_empty_bands_reach(key):
    p = pat(*key)
    gaps = set()
    for i, occ in enumerate(cp.occupied_bands(p.roi_h)):
        bands = table(p, i).sum(axis=(1, 2))
        assert np.flatnonzero(bands).tolist() == list(occ)
        gaps |= {b - a - 1 for a, b in zip(occ, occ[1:])}
    assert {1, 2} <= gaps and (p.ty < 130 or {63, 64, 65} <= gaps)


@pytest.mark.parametrize("key", of("tile_ramp"), ids=lambda k: "-".join(map(str, k)))
def test_tile_ramp_reach(key):
    """Tile t holds 1 + (t * 2654435761 % 13) survivors in each of its ramp rows and none elsewhere; every band and every
    tile column holds survivors -- band 128 and tile column 16 among them where the shape has them."""
    p = pat(*key)
    c = table(p, 0)
    want = np.zeros_like(c)
    for ty in range(p.ty):
        for tx in range(p.tx):
            w = min(cp.TW, p.roi_w - cp.TW * tx)
            for r in cp.ramp_rows_of(p.roi_w, p.k, tx):
                if cp.TH * ty + r < p.roi_h:
                    want[ty, r, tx] = min(w, cp.ramp_count(ty * p.tx + tx))
    assert np.array_equal(c, want)
    assert (c.sum(axis=(1, 2)) > 0).all() and (c.sum(axis=(0, 1)) > 0).all()
    assert len(set(want.max(axis=1).reshape(-1))) >= 8
    assert {r % 2 for tx in range(p.tx) for r in cp.ramp_rows_of(p.roi_w, p.k, tx)} == {0, 1}


def test_sliver_scales_are_what_they_are_meant_to_be():
    """Every non-zero byte decodes to a W below w_safe at both scales (the class-2 table entries that switch a block to the
    exact path); by the oracle nothing survives at the first and a part of the median's survivors at the second."""
    (c0, c1) = [c for c in CASES if c.scale != cp.SCALE]
    p, q = pattern_of(c0), d2pc.make_q()
    assert pattern_of(c1) is p
    w_safe = max(abs(q[11]), abs(q[3]), abs(q[3] + p.w), abs(q[7]), abs(q[7] + p.h)) * 2.0 ** -126
    for c in (c0, c1):
        d = (np.arange(1, 256, dtype=np.float32) * np.float32(c.scale)).astype(np.float64)
        assert (d > 0).all() and (np.abs(q[14] * d + q[15]) < w_safe).all()
        for i, med in enumerate(p.medians):
            pts, _ = oracle.reproject_compact(med, q, border=p.border, scale=c.scale)
            assert len(pts) == 0 if c is c0 else 0 < len(pts) < p.valid[i].sum(), (c.scale, i, len(pts))


# ------------------------------------------------------------------------------------------------ the oracle and the model
@pytest.mark.parametrize("key", KEYS, ids=IDS)
def test_valid_is_the_oracle_s_and_the_model_restates_it(key):
    """`Pattern.valid` against oracle.reproject_compact's own indices on every frame (the expected answer of the GPU file),
    and the model without a slip against np.flatnonzero(valid)."""
    p = pat(*key)
    pix = p.pix()
    for i, med in enumerate(p.medians):
        _, wi = oracle.reproject_compact(med, d2pc.make_q(), border=p.border, scale=p.scale, min_disparity=p.dmin)
        assert np.array_equal(wi, pix[np.flatnonzero(p.valid[i])]), (key, p.names[i])
        assert np.array_equal(cp.callback_model(p.valid[i], p.roi_w, p.roi_h), np.flatnonzero(p.valid[i])), (key, p.names[i])


@pytest.mark.parametrize("generator", cp.GENERATORS)
def test_fast_median_equals_the_checker_on_a_frame_of_each_generator(generator):
    for key in of(generator)[:2] + of(generator)[-1:]:
        p = pat(*key)
        assert np.array_equal(oracle.median_u8_fast(p.frames[0], p.k), p.medians[0]), key


# ------------------------------------------------------------------------------------------------------------ kill matrix
# Where a slip can occur at all: a property of the shape (and, for count_8bit, of the input).
CAN_OCCUR = {
    "count_8bit": lambda p: any((table(p, i) == 256).any() for i in range(len(p.frames))),
    "pair_swapped": lambda p: True,
    "left_includes_self": lambda p: True,
    "left_first_16_tiles": lambda p: p.tx > 16,
    "above_first_64": lambda p: p.ty > 65,
    "above_first_128": lambda p: p.ty > 129,
    "tail_cols_counted": lambda p: p.roi_w % cp.TW != 0,
    "tail_rows_counted": lambda p: p.roi_h % cp.TH != 0,
    "group_not_clipped": lambda p: p.roi_w % cp.GROUP != 0,
    "step_rank_restarts": lambda p: True,
    "band_total_for_count": lambda p: True,
}

# slip x generator over the patterns of the GPU file (X: the slip changes the model's output on every pattern of the
# generator, a number: on that many of them, a dot: on none)
KILL_MATRIX = """
slip                  row_counts   step_only    edges        tile_steps   empty_bands  tile_ramp
count_8bit            X            .            X            X            .            .
pair_swapped          X            X            X            X            X            X
left_includes_self    X            X            X            X            X            X
left_first_16_tiles   .            .            .            4            .            4
above_first_64        .            .            .            .            16           16
above_first_128       .            .            .            .            8            16
tail_cols_counted     X            X            X            8            12           16
tail_rows_counted     X            X            X            4            4            4
group_not_clipped     .            .            8            8            12           16
step_rank_restarts    X            .            X            X            16           X
band_total_for_count  .            .            X            X            X            X
"""

_kills = {}


def kills(key, slip):
    """Whether the slip changes the model's output on any frame of the pattern (equal masks are modelled once)."""
    p = pat(*key)
    hit = False
    for i, v in enumerate(p.valid):
        h = (hashlib.sha1(v.tobytes()).hexdigest(), hashlib.sha1(p.outside[i].tobytes()).hexdigest(), p.roi_w, p.roi_h, slip)
        if h not in _kills:
            _kills[h] = cp.killed(v, p.roi_w, p.roi_h, slip, p.outside[i])
        hit = hit or _kills[h]
    return hit


def matrix_text():
    lines = ["slip".ljust(22) + "".join(g.ljust(13) for g in cp.GENERATORS).rstrip()]
    for slip in cp.SLIPS:
        cells = []
        for g in cp.GENERATORS:
            k = [kills(key, slip) for key in of(g)]
            cells.append("X" if all(k) else str(sum(k)) if any(k) else ".")
        lines.append(slip.ljust(22) + "".join(c.ljust(13) for c in cells).rstrip())
    return "\n".join(lines)


def test_kill_matrix():
    got = matrix_text()
    print("\n" + got)
    assert got == KILL_MATRIX.strip("\n"), "\n" + got


@pytest.mark.parametrize("slip", cp.SLIPS)
def test_every_slip_is_killed_where_it_can_occur_and_nowhere_else(slip):
    """On a shape where the slip cannot occur the model's output is unchanged (the dots are proven, not assumed); among
    the shapes where it can, at least one pattern of the GPU file shows it -- and, for the shape-bound slips, at least
    one on EVERY such shape."""
    can = [key for key in KEYS if CAN_OCCUR[slip](pat(*key))]
    assert can, slip
    for key in KEYS:
        if key not in can:
            assert not kills(key, slip), (slip, key)
    assert any(kills(key, slip) for key in can), slip
    if slip != "count_8bit":
        for shape in {key[1] for key in can}:
            assert any(kills(key, slip) for key in can if key[1] == shape), (slip, shape)
