"""The built inputs of tests/window_cases.py on the CPU: every built fit cell is in a window that holds exactly its points at
the stated update, under the rules of the builder, and the reference's words there are the slope reference's and exact least
squares' decisions; every ring state's hand-stated outcome is both references' and ring_copy's; each mutation of ring_copy is
killed by the state named for it; each edge of the terrain's cell formula is reached, in exact integers.
tests/README_sectors_relief.md and tests/README_sectors_terrain.md have the maps.  No GPU."""
import numpy as np
import pytest

import slope_fit_cases as sfc
import window_cases as wc

K = 8
_runs = {}


# ------------------------------------------------------------------------------------------------ (a) fit cells in a window
def run_sequence(session, seq):
    """The relief reference over the sequence's frames -> its outputs, update by update."""
    if id(seq) not in _runs:
        ground, slope = session.config()
        ref = wc.relief_ref_of(ground, slope, seq.depth)
        _runs[id(seq)] = [ref.update(*unpack(seq.frame(f)), n_candidates=K) for f in seq.order]
    return _runs[id(seq)]


def unpack(step_and_tables):
    return (step_and_tables[0],) + tuple(step_and_tables[1])


def cell_words(w, t):
    """The reference's words for the window case's world cell at update t."""
    out = run_sequence(w.session, w.seq)[t]
    return wc.words_of(out, w.seq.n_a * w.seq.n_b, w.seq.index(t, w.b)), out


def slope_words(case):
    """SectorsSlopeRef.cells of the case's points alone in cell 0 of a grid of one."""
    p = np.asarray(case.points, dtype=np.int64)
    out = sfc.ref_of(sub=case.sub, n_a=1, n_b=1, **case.cfg).cells(np.zeros(len(p), dtype=np.int64), p[:, 2], p[:, 0], p[:, 1])
    return wc.words_of(out, 1, 0), out


def test_all_81_cells_are_built_and_share_sessions_by_key():
    cases = wc.window_cases()
    assert sorted(w.name for w in cases) == sorted([c.name for c in sfc.CASES] + [sfc.LOST.name]) and len(cases) == 81
    keys = [(s.fam, s.sub, tuple(sorted(s.cfg.items()))) for ss in wc.all_sessions().values() for s in ss]
    assert len(keys) == len(set(keys)), "one session a key"
    for fam in sfc.FAMILIES:
        assert [(s.sub, tuple(sorted(s.cfg.items()))) for s in wc.all_sessions()[fam]] == [k for k, _ in sfc.groups(fam)]
    grids = {(s.n_a, s.n_b) for ss in wc.all_sessions().values() for s in ss}
    assert grids == {(8, 3), (5, 3)} and 24 % 16 and 15 % 16, "no cell count is a multiple of 16: the last block is partly filled"
    assert [w.session.n_a for w in cases if w.name.endswith("_of_7")] == [5, 5, 5]


def test_the_four_rules_hold_for_every_case():
    for w in wc.window_cases():
        seq, b = w.seq, w.b
        for t in w.updates:
            held = [seq.tracks[b].part(f) for f in range(max(0, t - seq.depth + 1), t + 1)]
            # 1. at least three frames hold the case's points (as many as it has points, for the two smallest)
            assert sum(1 for p in held if p) >= min(3, len(w.case.points)), (w.name, "rule 1")
            assert len(held) >= 3 and run_sequence(w.session, seq)[t]["status"][1] == len(held), (w.name, "every frame of the window took part")
            # 3. the window holds the case's points and no other (from the frames alone)
            pts, shifts = seq.window_points(b, t)
            assert pts == sorted(w.case.points), (w.name, "rule 3")
            assert (0, 0) not in shifts and len(set(shifts)) == len(shifts), (w.name, "every stored table is read at a shifted index")
        # 2. over the updates up to the stated one the shifts take both signs on both axes, and one is n_a - 1 or n_b - 1
        shifts = [s for t in range(max(w.updates) + 1) for s in seq.window_points(b, t)[1]]
        da, db = [d for d, _ in shifts], [d for _, d in shifts]
        assert min(da) < 0 < max(da) and min(db) < 0 < max(db), (w.name, "rule 2: both signs on both axes")
        assert seq.n_a - 1 in map(abs, da) or seq.n_b - 1 in map(abs, db), (w.name, "rule 2: a shift of n - 1")
        # 4. an earlier update gave other words: the window gave the answer, not one frame
        final = cell_words(w, w.updates[0])[0]
        assert any(cell_words(w, t)[0] != final for t in range(w.updates[0])), (w.name, "rule 4")


def test_every_session_has_a_case_on_the_seam_of_two_blocks_and_in_the_last_block():
    for ss in wc.all_sessions().values():
        for s in ss:
            if s.n_a * s.n_b <= 16:
                continue
            index = {seq.index(f, b) for seq in s.sequences[:1] for f in range(3) for b in range(len(seq.tracks))}
            assert {15, 16} <= index, "index 15 ends block 0 of k_relief_window, index 16 begins block 1, the last one, of 8 cells"


def test_the_window_s_words_are_the_slope_reference_s_and_exact_least_squares_decisions():
    not_equal = []
    for w in wc.window_cases():
        c, e = w.case, w.case.exact()
        want, _ = slope_words(c)
        for t in w.updates:
            got, out = cell_words(w, t)
            assert got == want, (w.name, t, "the fit from the window's sums is the fit from the case's points")
            cell = w.seq.index(t, w.b)
            fitted, flat, level, resid = int(out["fitted"][cell]), int(out["flat"][cell]), int(out["level_q"][cell]), int(out["resid_q2"][cell])
            assert (fitted, flat) == (int(e["fitted"]), int(e["flat"])), w.name
            assert int(out["site"][cell]) == flat, "a window of 0: a flat cell is a site"
            for what, value in c.expect.items():
                if what != "q_sign":
                    assert dict(fitted=fitted, flat=flat, level_q=level, resid_q2=resid)[what] == value, (w.name, what)
            if c.family in ("tilt", "level") or (c.family == "resid" and "just" not in c.name):      # where test_slope_fit_cases asserts equality
                assert (level, resid) == (e["level_q"], e["resid_q2"]), w.name
                if e["fitted"]:
                    assert (np.uint32(got[3]).view(np.float32), np.uint32(got[4]).view(np.float32)) == (e["slope_a"], e["slope_b"]), w.name
            if (level, resid) != (e["level_q"], e["resid_q2"]):
                not_equal.append(w.name)
    assert sorted(set(not_equal)) == ["lost_level_tie"], "as measured in tests/test_slope_fit_cases.py"
    lost = next(w for w in wc.window_cases() if w.name == "lost_level_tie")
    assert cell_words(lost, 2)[0][5] == 2 and sfc.LOST.exact()["level_q"] == 1


def test_every_eviction_pair_flips_its_decision_between_two_consecutive_updates():
    by = {w.name: w for w in wc.window_cases()}
    tracks = [(s, seq, b) for ss in wc.all_sessions().values() for s in ss for seq in s.sequences for b in range(len(seq.tracks))]
    field = dict(fitted=lambda out, c: int(out["fitted"][c]), flat=lambda out, c: int(out["flat"][c]), level_q=lambda out, c: int(out["level_q"][c]))
    for before, after, what in wc.eviction_pairs():
        session, seq, b = next(x for x in tracks if after in x[1].tracks[x[2]].at and (before is None or before in x[1].tracks[x[2]].at))
        track, w = seq.tracks[b], by[after]
        w = type(w)(w.case, session, seq, b)                          # (the track that holds both: rule 3 is asserted again)
        if before is not None:
            t = next(u for u in track.at[after] if u - 1 in track.at[before])
            assert seq.window_points(b, t - 1)[0] == sorted(by[before].case.points) and abs(len(by[before].case.points) - len(w.case.points)) <= 2
        else:
            t = track.at[after][0]
            assert t - 1 in track.unnamed and seq.window_points(b, t - 1)[0] == sorted(track.unnamed[t - 1])
        runs = run_sequence(session, seq)
        a, b = field[what](runs[t - 1], w.seq.index(t - 1, w.b)), field[what](runs[t], w.seq.index(t, w.b))
        print("%s -> %s: %s %d -> %d at updates %d, %d" % (before or "(its rough neighbour)", after, what, a, b, t - 1, t))
        assert a != b, (before, after, what)
        if what == "flat":                                            # the rough neighbour is one quantum^2 or more above the bound
            c = w.seq.index(t - 1, w.b)
            assert runs[t - 1]["fitted"][c] and runs[t - 1]["resid_q2"][c] > w.case.cfg["max_spread_q2"] == runs[t]["resid_q2"][w.seq.index(t, w.b)], after
    # the gate pairs at the updates the issue names, on their own
    one = by["gate_one_off_fails"]
    assert one.updates == [3] and by["gate_one_off_holds"].updates == [4] and one.depth == 4
    assert [len(p) for p in one.track.parts] == [2, 9320, 1, 9320, 0], "the extra point a cluster, one cluster, the point off the diagonal, the other cluster, nothing"
    assert [len(one.seq.window_points(one.b, t)[0]) for t in (3, 4)] == [18643, 18641]
    assert [by["gate_count_%s" % n].updates for n in ("4_of_3", "3_of_3", "2_of_3", "8_of_7", "7_of_7", "6_of_7")] == [[3], [4], [4]] * 2
    for tag in sfc.LEVEL_TIES:
        assert [by["level_%s_%s" % (tag, x)].updates for x in ("down", "tie", "up")] == [[3], [4, 7], [8]], "the moved height enters and leaves"


# ------------------------------------------------------------------------------------------------ (b) ring states
def run_state(kind, st):
    """The reference of `kind` from the planted state over the one frame -> (outputs, the state block after, count, planes)."""
    ref = wc.relief_ref_of(st.ground(), dict(sub=8, max_slope=sfc.MAX_SLOPE), st.depth) if kind == "relief" else wc.terrain_ref_of(st.ground(), st.depth)
    ref.state[:] = st.render(kind)
    out = ref.update(st.step(), *st.frame(kind), n_candidates=K)
    n = st.n_a * st.n_b
    planes = [np.asarray(out["sum"]).view(np.uint64), np.asarray(out["sum2"]).view(np.uint64)]
    if kind == "relief":
        planes += list(np.asarray(out["moments"]).view(np.uint64).reshape(7, n))
    return out, ref.state.copy(), np.asarray(out["count"]), planes


@pytest.mark.parametrize("kind", ["relief", "terrain"])
def test_the_hand_stated_outcome_of_every_ring_state_is_the_reference_s(kind):
    states = wc.all_ring_states()
    assert len({st.name for st in states}) == len(states) == 26
    for st in states:
        out, after, count, planes = run_state(kind, st)
        wc.check_state(kind, st, count, planes, out["status"], after, "%s, %s" % (kind, st.name))
    by = {st.name: st for st in states}
    assert [by["smallest_at_%d" % x].v for x in (0, 7, 15)] == [0, 7, 15] and (by["tie_of_two"].v, by["tie_of_five"].v) == (4, 3)
    assert len(by["fifteen_take_part"].parts) == 15 and len({p[1:] for p in by["fifteen_take_part"].parts}) == 15
    assert (len(by["depth_2_full"].parts), len(by["depth_9_full"].parts)) == (1, 8)
    assert [[p[0] for p in by[n].parts] for n in ("holes_alternating", "holes_only_the_last", "holes_only_the_first", "holes_none_nan")] == [
        [1, 3, 5, 7, 9, 11, 13, 15], [15], [0], []] and [p[0] for p in by["all_but_slot_1"].parts] == [0] + list(range(2, 16))
    n_a, n_b = by["edge_of_sight"].n_a, by["edge_of_sight"].n_b
    shifts = {p[1:] for p in by["edge_of_sight"].parts}
    assert {(n_a - 1, 0), (-(n_a - 1), 0), (0, n_b - 1), (0, -(n_b - 1)), (0, 0)} <= shifts and not any(abs(d) >= n_a or abs(e) >= n_b for d, e in shifts)
    low = by["extreme_anchors_low"]
    assert min(low.headers[0][0], low.headers[1][1]) == -(1 << 31) and abs(int(low.corner[0]) - low.headers[1][0]) >= 1 << 31, "more than 32 bits"
    assert all(h[3] != 0 and h[2] == wc.H_ONE for h in by["beyond_depth_update"].headers[3:]), "loud headers beyond depth"


def test_the_signature_decodes_what_was_added_and_names_what_was_not():
    st = next(s for s in wc.all_ring_states() if s.name == "edge_of_sight")
    for kind in ("relief", "terrain"):
        _, _, count, planes = run_state(kind, st)
        corner = wc.decode(kind, count, planes, 0)
        assert (wc.FRAME_ENTRY, 0) in corner and (0, st.n_a - 1) in corner and (12, st.n_a * st.n_b - 1) in corner, "read at the shifted index"
        planes[0][3] += np.uint64(1) << np.uint64(wc.layout(kind)[0] * 4)                         # as if slot 4 had been added
        with pytest.raises(AssertionError, match="cell 3, entry 4"):
            wc.decode(kind, count, planes, 3, kind)


# ------------------------------------------------------------------------------------------------ (c) the ring, with its operators
def copy_of(st, ops=None):
    return wc.ring_copy(st.headers, st.depth, st.n_a, st.n_b, st.corner, st.h0, inv_c=1.0 / st.cell, ops=ops)


def test_ring_copy_is_both_references_on_every_state_and_on_200_random_ones():
    rng = np.random.default_rng(31)
    states = wc.all_ring_states() + [wc.random_state(rng) for _ in range(200)]
    seen = dict(restart=0, unanchored=0, full=0, none=0)
    for n, st in enumerate(states):
        r = copy_of(st)
        if st.name != "random":                                       # the hand-stated outcome is the copy's
            assert (r["anchored"], r["restart"], r["v"], r["q"], r["parts"]) == (st.anchored, st.restart, st.v, st.q, st.parts), st.name
        for kind in ("relief", "terrain"):
            out, after, count, planes = run_state(kind, st)
            what = "%s, %s %d" % (kind, st.name, n)
            assert [int(x) for x in out["status"]] == r["status"], what
            assert [[int(x) for x in h] for h in after[:256].view(np.uint32).reshape(16, 4)] == [[x & wc.M32 for x in h] for h in r["headers"]], what
            want = wc.hand_window(st.n_a, st.n_b, r["parts"], r["anchored"])
            assert all(wc.decode(kind, count, planes, c, what) == want[c] for c in range(st.n_a * st.n_b)), what
        seen["restart"] += r["restart"]
        seen["unanchored"] += not r["anchored"]
        seen["full"] += r["anchored"] and len(r["parts"]) == st.depth - 1 and st.depth > 1
        seen["none"] += r["anchored"] and not r["parts"]
    assert min(seen.values()) >= 3, seen


# the state built for each mutation, asserted to be among those that kill it
RING_KILLERS = {
    "anchor < for <=": ("extreme_anchors_low", "extreme_anchors_high"),
    "di > -n_a: >= for >": ("out_at_minus_n_a", "edge_of_sight"),
    "di < n_a: <= for <": ("out_at_plus_n_a", "edge_of_sight"),
    "dj > -n_b: >= for >": ("out_at_minus_n_b", "edge_of_sight"),
    "dj < n_b: <= for <": ("out_at_plus_n_b", "edge_of_sight"),
    "ia0 - h.x negated": ("fifteen_take_part", "edge_of_sight", "depth_2_full"),
    "di and dj exchanged": ("fifteen_take_part", "edge_of_sight", "depth_2_full"),
    "the highest index on a tie": ("tie_of_two", "tie_of_five", "holes_alternating"),
    "signed compare of seq": ("large_seqs", "seq_fffffffe"),
    "seq != 0 dropped": ("holes_alternating", "holes_only_the_last"),
    "slot != v dropped": ("all_but_slot_1", "smallest_at_7"),
    "h0 compared as bits": ("holes_alternating", "holes_none_nan"),
    "restart at largest >= 0xFFFFFFFE": ("seq_fffffffe",),
    "q = largest without + 1": ("smallest_at_0", "large_seqs", "depth_9_full"),
}
# ia0 and jb0 are at most 2^29 in size and a stored anchor at most 2^31: a difference d has |d| <= 2^29 + 2^31 < 2^32, and one
# that 32 bits do not hold wraps to d -+ 2^32, of size 2^31 - 2^29 at least: out of sight either way, for any grid (n_a, n_b <= 64).
# No state can tell the two; the 64-bit difference stays, as the specification words it.
EQUIVALENT = ("32-bit wrap of di",)


@pytest.mark.parametrize("name", list(wc.RING_MUTATIONS))
def test_each_mutation_of_the_ring_is_killed_by_the_state_named_for_it(name):
    rng = np.random.default_rng(32)
    states = wc.all_ring_states()
    killed = [st.name for st in states if copy_of(st, wc.RING_MUTATIONS[name]) != copy_of(st)]
    at_random = sum(copy_of(st, wc.RING_MUTATIONS[name]) != copy_of(st) for st in (wc.random_state(rng) for _ in range(200)))
    print("%s: killed by %d states (and %d of 200 random ones): %s" % (name, len(killed), at_random, ", ".join(killed)))
    if name in EQUIVALENT:
        assert not killed and not at_random, "a state now tells the 32-bit difference from the 64-bit one: take it off EQUIVALENT"
        extreme = [st for st in states if st.name.startswith("extreme")]
        assert any(abs(int(st.corner[0]) - h[0]) >= 1 << 31 for st in extreme for h in st.headers), "a difference that 32 bits do not hold is built"
        return
    assert killed, "no state kills it"
    assert set(RING_KILLERS[name]) <= set(killed), "the states built for this edge"


# ------------------------------------------------------------------------------------------------ (d) the terrain's cell formula
def run_edge(e):
    ref = wc.terrain_ref_of(e.ground(), e.depth)
    return [ref.update(*unpack(e.frame(f)), n_candidates=K) for f in range(len(e.frames))]


def test_each_edge_of_the_terrain_s_cell_formula_is_reached_in_exact_integers():
    edges = {e.name: e for e in wc.terrain_edges()}
    for e in edges.values():
        assert len(e.frames) >= 3 and len({f[0] for f in e.frames[:3]}) == 3, "three or more frames, each at a corner of its own"
        wc.check_edge(e, run_edge(e), "the reference,")
    x = edges["min_count_by_the_window"].expect
    assert [(x[t][wc.W0]["count"], x[t][wc.W0]["flat"]) for t in range(4)] == [(2, 0), (4, 0), (6, 1), (5, 0)] and edges["min_count_by_the_window"].cfg["min_count"] == 6
    x = edges["spread_at_and_above_the_bound"].expect
    assert [(x[t][wc.W0]["spread_q2"], x[t][wc.W0]["flat"]) for t in (2, 3)] == [(625, 1), (626, 0)] and x[2][wc.W0]["S"] == 625 * 6
    x = edges["floor_mean_of_a_negative_sum"].expect
    for t, (total, n, floor, trunc) in ((1, (-65533, 2, -32767, -32766)), (2, (-65533, 4, -16384, -16383)), (3, (-98294, 6, -16383, -16382))):
        assert (x[t][wc.W0]["sum"], x[t][wc.W0]["count"], x[t][wc.W0]["mean_q"]) == (total, n, floor) and total % n and sfc.trunc_mean(total, n) == trunc
    e = edges["step_at_and_above_the_bound"]
    nb = (wc.W0[0] + 1, wc.W0[1])
    assert [e.expect[t][wc.W0]["mean_q"] - e.expect[t][nb]["mean_q"] for t in (2, 3, 4)] == [40, 41, 40] and e.cfg["max_step_q"] == 40 and e.cfg["window"] == 1
    assert [(e.expect[t][wc.W0]["site"], e.expect[t][nb]["site"]) for t in (2, 3, 4)] == [(1, 1), (0, 0), (1, 1)]
    assert all(e.expect[t][c]["flat"] == 1 for t in (2, 3, 4) for c in (wc.W0, nb)), "every cell stays flat: the step alone takes the sites"
    e = edges["largest_window"]
    for cell, sign in ((wc.W0, 1), (nb, -1)):
        w = e.expect[15][cell]
        assert w["count"] == 4294967280 == 16 * 268435455 < 1 << 32 and w["mean_q"] == sign * 32766 and w["S"] == w["count"] and w["spread_q2"] == 1
        sum2 = sum(h * h * k for f in e.frames for h, k in f[1][cell])
        um, us = w["mean_q"] & wc.M64, w["sum"] & wc.M64
        if sign < 0:
            assert w["count"] * um * um >= 1 << 64 and 2 * um * us >= 1 << 64, "as 64-bit words both products pass 2^64 and wrap"
            assert sfc.trunc_mean(w["sum"], w["count"]) == -32765, "the truncated mean is another"
        else:
            assert sum2 - 2 * um * us < 0 and 2 * um * us + w["count"] * um * um >= 1 << 63, "the difference wraps below zero"
        assert (sum2 - 2 * um * us + w["count"] * um * um) & wc.M64 == w["S"] < 1 << 64, "the wrapped formula still gives S"
