"""The built inputs of tests/window_cases.py through d2pc_sectors_relief_update_device: every built fit cell of
tests/slope_fit_cases.py spread over a window of depth 4 (one test a family), and the planted ring states (one test a group).
Every update's thirteen outputs and the state block behind it are the bytes of tests/sectors_relief_ref.py (sentinel-filled,
16 guard entries: the harness of tests/test_sectors_relief_gpu.py); the decision each case names has its stated value in the
DEVICE's output at the stated update; from the device's sums alone the signature tells which (slot, cell) pairs were added.
tests/test_window_cases.py proves on the CPU that the inputs reach their edges; tests/README_sectors_relief.md has the map and,
for each test, the mutation it is there to catch."""
import numpy as np
import pytest

import sectors_slope_ref as sref
import slope_fit_cases as sfc
import window_cases as wc
from test_sectors_relief_gpu import NONE, Harness, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 8
_made = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sessions():
    yield
    for h in _made.values():
        h.close()
    _made.clear()


def harness(depth, ground, slope):
    key = (depth, tuple(sorted(ground.items())), tuple(sorted(slope.items())))
    if key not in _made:
        _made[key] = Harness(depth, sub=slope["sub"], max_slope=slope["max_slope"], **ground)
    return _made[key]


def run(h, step, frame, what):
    """One update of the device and of the reference -> the DEVICE's outputs, which are the reference's bytes, as the state is."""
    step = np.asarray(step, dtype=np.uint32)
    got = h.device(step, frame, None, K)
    exp = h.ref.update(step, *frame, n_candidates=K)
    same(got, exp, what)
    state = h.read_state()
    bad = np.flatnonzero(state != h.ref.state)
    assert bad.size == 0, "%s: state byte %d is %#x, not %#x (%d differ)" % (what, bad[0], state[bad[0]], h.ref.state[bad[0]], bad.size)
    return got


# ------------------------------------------------------------------------------------------------ (a) fit cells in a window
def books(got, what):
    """The device's site, candidates and summary follow from the device's own per-cell bytes (a window of 0, at most K sites)."""
    fitted = got["slope_a"] != sref.NOT_FITTED
    assert np.array_equal(got["site"], got["flat"]), "%s: a window of 0: a flat cell is a site" % what
    assert got["summary"].tolist() == [int(got["count"].astype(np.uint64).sum()), int(got["flat"].sum()), int(got["site"].sum()), int(fitted.sum())], what
    listed = sorted(int(c) & 0xFFFFFFFF for c in got["candidates"] if c != NONE)
    assert listed == np.flatnonzero(got["site"]).tolist(), "%s: the candidates are the sites" % what
    return fitted


def run_sequence(h, seq, what):
    h.reset()
    outs = []
    for n, f in enumerate(seq.order):
        step, frame = seq.frame(f)
        outs.append(run(h, step, frame, "%s, update %d (frame %d)" % (what, n, f)))
        assert outs[-1]["status"].tolist() == [n + 1, min(n + 1, seq.depth), seq.corners[f][0] & wc.OFF, seq.corners[f][1] & wc.OFF]
    return outs


def value_of(got, cell):
    return dict(fitted=int(got["slope_a"][cell] != sref.NOT_FITTED), flat=int(got["flat"][cell]), level_q=int(got["level_q"][cell]),
                resid_q2=int(got["resid_q2"][cell]), site=int(got["site"][cell]))


def run_family(fam):
    """Every sequence of every session of the family, every update compared -> {case name: the device's values at its update}."""
    seen, outs = {}, {}
    for s in wc.all_sessions()[fam]:
        ground, slope = s.config()
        h = harness(wc.DEPTH, ground, slope)
        for n, seq in enumerate(s.sequences):
            outs[id(seq)] = run_sequence(h, seq, "%s, sub %d, %s, sequence %d" % (fam, s.sub, s.cfg, n))
            for t, got in enumerate(outs[id(seq)]):
                books(got, "%s, update %d" % (fam, t))
        for w in s.window_cases:
            e = w.case.exact()
            for t in w.updates:
                got, cell = outs[id(w.seq)][t], w.seq.index(t, w.b)
                value = value_of(got, cell)
                assert got["count"][cell] == len(w.case.points), w.name
                assert (value["fitted"], value["flat"]) == (int(e["fitted"]), int(e["flat"])), "%s: exact least squares decides otherwise" % w.name
                for name, stated in w.case.expect.items():
                    if name != "q_sign":
                        assert value[name] == stated, "%s: %s is %d on the device at update %d, stated %d (%s)" % (w.name, name, value[name], t, stated, w.case.edge)
                seen[w.name] = value
    # the pairs that eviction reaches: the decision flips between two consecutive updates, and the books follow the byte
    for s, seq, b, t, before, after, what in wc.located_pairs(fam):
        a, c = outs[id(seq)][t - 1], outs[id(seq)][t]
        va, vc = value_of(a, seq.index(t - 1, b)), value_of(c, seq.index(t, b))
        assert va[what] != vc[what], "%s -> %s: %s stays %d on the device" % (before, after, what, va[what])
        assert (va["site"], vc["site"]) == (va["flat"], vc["flat"])
        for got, v, cell in ((a, va, seq.index(t - 1, b)), (c, vc, seq.index(t, b))):
            assert (cell in {int(x) & 0xFFFFFFFF for x in got["candidates"] if x != NONE}) == bool(v["site"]), (before, after, "candidates")
        seen[(before, after)] = (va, vc)
    return seen, outs


def test_gate_cases_in_a_window_and_the_same_window_in_the_reverse_order_of_arrival():
    """Catches, of the scratch builds: `cnt > min_fit`-like changes of slope_cell_fit's gate in k_relief_window's copy, the sign of
    di and `<=` for `<` in terrain_participants (a frame read at the wrong shift, or not at all, changes N about the gate)."""
    seen, outs = run_family("gate")
    assert [seen["gate_%s" % n]["fitted"] for n in ("one_off_fails", "one_off_holds", "two_off_fails", "two_off_holds", "d_zero", "a_zero")] == [0, 1, 0, 1, 0, 0]
    assert [seen["gate_count_%s" % n]["fitted"] for n in ("2_of_3", "3_of_3", "4_of_3", "6_of_7", "7_of_7", "8_of_7")] == [0, 1, 1, 0, 1, 1]
    assert seen[("gate_one_off_fails", "gate_one_off_holds")][0]["fitted"] == 0 and seen[("gate_one_off_fails", "gate_one_off_holds")][1]["fitted"] == 1
    # the window of updates 3 and 4 once more, its frames arriving in the reverse order: the same window gives the same bytes
    for s in wc.all_sessions()["gate"]:
        h = harness(wc.DEPTH, *s.config())
        n = s.n_a * s.n_b
        for seq in s.sequences:
            for t in (3, 4):
                rev = seq.reversed_window(t)
                last = run_sequence(h, rev, "gate, the window of update %d reversed" % t)[-1]
                for b in range(len(seq.tracks)):
                    forward = wc.words_of(outs[id(seq)][t], n, seq.index(t, b))
                    assert wc.words_of(last, n, rev.index(rev.order[-1], b)) == forward, "track %d: the reversed window of update %d gives other bytes" % (b, t)


def test_tilt_cases_in_a_window_move_the_sites_and_the_summary():
    """Catches `<` for `<=` in the tilt test of k_relief_window's slope_cell_fit, and a contracted or reordered sa sa + sb sb."""
    seen, _ = run_family("tilt")
    for axis in "uw":
        assert [seen["tilt_%s_%s" % (axis, tag)]["flat"] for tag in ("at", "below", "above")] == [1, 0, 1]
        assert [seen["tilt_%s_%s" % (axis, tag)]["site"] for tag in ("at", "below", "above")] == [1, 0, 1]
    assert (seen["tilt_both_below"]["flat"], seen["tilt_both_above"]["flat"]) == (0, 1)


def test_resid_cases_in_a_window_reached_from_a_rough_neighbour():
    """Catches `<` for `<=` in the residual test and a Q formed otherwise than (G - gu E) - gw F in k_relief_window's copy."""
    seen, _ = run_family("resid")
    for d in (1, 25, 181):
        at, under = seen["resid_d%d_at" % d], seen["resid_d%d_under" % d]
        assert at["resid_q2"] == under["resid_q2"] == d * d and (at["flat"], under["flat"]) == (1, 0) and (at["site"], under["site"]) == (1, 0)
        rough, flat = seen[(None, "resid_d%d_at" % d)]
        assert rough["resid_q2"] > d * d == flat["resid_q2"] and (rough["flat"], flat["flat"]) == (0, 1)
    assert seen["resid_just_below"]["resid_q2"] == seen["resid_just_above"]["resid_q2"] == 627
    assert (seen["resid_just_below"]["flat"], seen["resid_just_above"]["flat"]) == (1, 0)
    wide = sfc.by_name("resid_wide").exact()
    assert seen["resid_wide"]["resid_q2"] == wide["resid_q2"] > 29000 ** 2 and seen["resid_wide"]["level_q"] == wide["level_q"]


def test_level_cases_in_a_window_round_the_tie_to_the_even_c0():
    """Catches `trunc` for `rint` (and half up) in k_relief_window's slope_cell_fit: the moved height enters and leaves."""
    seen, _ = run_family("level")
    for tag, (c0, _, m, rc) in sfc.LEVEL_TIES.items():
        for name, shift in (("tie", 0), ("neg", -32000), ("negodd", -32001), ("pos", 32000)):
            assert seen["level_%s_%s" % (tag, name)]["level_q"] == m + shift + rc, (tag, name)
        assert seen["level_%s_down" % tag]["level_q"] <= seen["level_%s_tie" % tag]["level_q"] <= seen["level_%s_up" % tag]["level_q"]
        assert seen["level_%s_down" % tag]["level_q"] < seen["level_%s_up" % tag]["level_q"]
    assert seen["lost_level_tie"]["level_q"] == 2, "the doubles' c0 lies just above -1.5 (exact least squares: 1)"


def test_thirds_cases_in_a_window_clamp_a_negative_q():
    """Catches a Q of another sign: a contracted multiply-add in gu E or gw F changes the rounding residue these cells live on."""
    seen, _ = run_family("thirds")
    for c in sfc.family("thirds"):
        assert seen[c.name]["fitted"] == 1 and seen[c.name]["resid_q2"] == 0 and seen[c.name]["level_q"] == c.exact()["level_q"], c.name


def test_noise_cases_in_a_window_are_the_reference_s_bytes():
    """Catches any reordered product or contraction in the second instance of the fit: every slope is the float32 of a double."""
    seen, _ = run_family("noise")
    for c in sfc.family("noise"):
        e = c.exact()
        assert (seen[c.name]["level_q"], seen[c.name]["resid_q2"], seen[c.name]["flat"]) == (e["level_q"], e["resid_q2"], int(e["flat"])), "exact least squares', as on the CPU"


# ------------------------------------------------------------------------------------------------ (b) ring states
SLOPE = dict(sub=8, max_slope=sfc.MAX_SLOPE)


def run_state(st):
    h = harness(st.depth, st.ground(), SLOPE)
    what = "relief, %s (%d x %d, depth %d)" % (st.name, st.n_a, st.n_b, st.depth)
    h.plant_state(st.render("relief"))
    got = run(h, st.step(), st.frame("relief"), what)
    n = st.n_a * st.n_b
    planes = [got["sum"].view(np.uint64), got["sum2"].view(np.uint64)] + list(got["moments"].view(np.uint64).reshape(7, n))
    wc.check_state("relief", st, got["count"], planes, got["status"], h.read_state(), what)
    return got


def run_group(*prefixes):
    states = [st for st in wc.all_ring_states() if st.name.startswith(prefixes)]
    assert states
    return {st.name: run_state(st) for st in states}


def test_ring_states_of_the_slot_choice():
    """Catches the highest index on a tie in terrain_slot_choice, a signed compare of seq, a restart at 0xFFFFFFFE, q without + 1."""
    got = run_group("smallest_at", "tie_of", "large_seqs", "seq_ff")
    assert len(got) == 8 and got["seq_ffffffff"]["status"].tolist()[:2] == [1, 1] and got["seq_fffffffe"]["status"][0] == 0xFFFFFFFF


def test_ring_states_at_the_edge_of_sight_with_fifteen_participants():
    """Catches `<=` for `<` (and `>=` for `>`) in each in-sight comparison of terrain_participants, the sign of di, di and dj
    exchanged, and a list position e - 1 mapped to another slice than e in k_relief_window."""
    got = run_group("fifteen", "edge_of_sight", "out_at")
    assert got["fifteen_take_part"]["status"][1] == 16 and got["edge_of_sight"]["status"][1] == 8 and all(got[n]["status"][1] == 15 for n in got if n.startswith("out_at"))
    big = next(st for st in wc.ring_states(46, 46) if st.name == "fifteen_take_part")      # the one 46 x 46: the last block holds 4 cells
    assert run_state(big)["status"][1] == 16


def test_ring_states_with_holes_in_the_list():
    """Catches `seq != 0` dropped, h0 compared as bits, and a compaction whose prefix popcount goes wrong where pos != lane."""
    got = run_group("holes_", "all_but_slot_1")
    assert [int(got[n]["status"][1]) for n in ("holes_alternating", "holes_only_the_last", "holes_only_the_first", "holes_none_nan", "all_but_slot_1")] == [9, 2, 2, 1, 16]


def test_ring_states_at_other_depths_beyond_the_depth_and_at_extreme_anchors():
    """Catches a header at or beyond `depth` read or written (an update, a restart, an unanchored frame), part_n == depth - 1 at
    depth 2 and 9, the anchor's `<=`, and a difference of anchors formed in 32 bits that came into sight."""
    got = run_group("depth_", "beyond_depth", "extreme_anchors")
    assert got["beyond_depth_unanchored"]["status"].tolist() == [5, 0, 0, 0] and got["beyond_depth_restart"]["status"].tolist()[:2] == [1, 1]
    assert (got["depth_2_full"]["status"][1], got["depth_9_full"]["status"][1]) == (2, 9) and got["extreme_anchors_low"]["status"][1] == 2
