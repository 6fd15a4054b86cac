"""The built inputs of tests/window_cases.py through d2pc_sectors_terrain_update_device: the planted ring states (one test a
group, the groups of tests/test_sectors_relief_values_gpu.py: the headers are the same, only the tables differ) and the
window-only edges of the GROUND block's cell formula.  Every update's ten outputs and the state block behind it are the bytes of
tests/sectors_terrain_ref.py (sentinel-filled, 16 guard entries: the harness of tests/test_sectors_terrain_gpu.py); from the
device's count, sum and sum2 alone the signature tells which (slot, cell) pairs were added; each edge's integers, worked out by
hand, are in the DEVICE's output.  tests/test_window_cases.py proves on the CPU that the inputs reach their edges;
tests/README_sectors_terrain.md has the map and, for each test, the mutation it is there to catch."""
import numpy as np
import pytest

import window_cases as wc
from test_sectors_terrain_gpu import Harness, same

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


def harness(depth, ground):
    key = (depth, tuple(sorted(ground.items())))
    if key not in _made:
        _made[key] = Harness(depth, **ground)
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


# ------------------------------------------------------------------------------------------------ (b) ring states
def run_state(st):
    h = harness(st.depth, st.ground())
    what = "terrain, %s (%d x %d, depth %d)" % (st.name, st.n_a, st.n_b, st.depth)
    h.plant_state(st.render("terrain"))
    got = run(h, st.step(), st.frame("terrain"), what)
    wc.check_state("terrain", st, got["count"], [got["sum"].view(np.uint64), got["sum2"].view(np.uint64)], got["status"], h.read_state(), what)
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
    exchanged, and a list entry added at another slot's shift in k_terrain_update."""
    got = run_group("fifteen", "edge_of_sight", "out_at")
    assert got["fifteen_take_part"]["status"][1] == 16 and got["edge_of_sight"]["status"][1] == 8 and all(got[n]["status"][1] == 15 for n in got if n.startswith("out_at"))


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


# ------------------------------------------------------------------------------------------------ (d) the cell formula
def test_window_only_edges_of_the_cell_formula():
    """Catches, in k_terrain_update's cell formula on the WINDOW's sums: `>` for `>=` at min_count, `<` for `<=` at max_spread_q2
    and at max_step_q, a truncated mean for the floor mean, and a spread sum formed in fewer than 64 wrapping bits."""
    for e in wc.terrain_edges():
        h = harness(e.depth, e.ground())
        h.reset()
        outs = []
        for f in range(len(e.frames)):
            step, frame = e.frame(f)
            outs.append(run(h, step, frame, "%s, update %d" % (e.name, f)))
            assert outs[-1]["status"].tolist()[:2] == [f + 1, min(f + 1, e.depth)]
        wc.check_edge(e, outs, "the device,")
