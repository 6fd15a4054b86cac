"""The built cells of tests/slope_fit_cases.py through d2pc_sectors_slope_process_device: one test per family, every case of
a session in a cell of its own on one small grid of one cloud.  Each asserts that the twelve outputs are the bytes of
tests/sectors_slope_ref.py (sentinel-filled, 16 guard entries: the harness of tests/test_sectors_slope_gpu.py), that the
decision each case names has its stated value in the DEVICE's output, and that the same records shuffled and cut into two
clouds at an odd record give the same bytes.  tests/test_slope_fit_cases.py proves on the CPU that the cases reach their
edges; tests/README_sectors_slope.md has the map."""
import numpy as np
import pytest

import sectors_slope_ref as sref
import slope_fit_cases as sfc
from test_sectors_slope_gpu import DTYPE, NONE, OUT, PT_SENTINEL, Harness, records, same

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

K = 5
_made = {}


@pytest.fixture(scope="module", autouse=True)
def _close_sessions():
    yield
    for h in _made.values():
        h.close()
    _made.clear()


def session(sub, n_a, n_b, cfg, **more):
    key = (sub, n_a, n_b, tuple(sorted(cfg.items())), tuple(sorted(more.items())))
    if key not in _made:
        _made[key] = Harness(sub=sub, max_slope=cfg["max_slope"], n_a=n_a, n_b=n_b, cell_size=sfc.CELL_SIZE, quantum=sfc.QUANTUM, window=0,
                             min_count=cfg["min_count"], max_spread_q2=cfg["max_spread_q2"], **more)
    return _made[key]


def shuffled_in_two_clouds(words, seed):
    """The records in another order, cut at an odd record into two clouds a stride apart; what lies between holds NaNs."""
    n = len(words)
    first = (n // 2) | 1
    cp = max(first, n - first)
    buf = np.full((2 * cp, words.shape[1]), 0x12345678, dtype=np.uint32)
    buf[:, :3] = PT_SENTINEL
    mixed = words[np.random.default_rng(seed).permutation(n)]
    buf[:first], buf[cp:cp + n - first] = mixed[:first], mixed[first:]
    return buf, cp, [first, n - first]


def run_family(fam, extra=(), **more):
    """Every session of the family -> {case name: what the device gave for its cell and for the call}."""
    seen = {}
    for (sub, items), cases in sfc.groups(fam):
        cfg = dict(items)
        cases = cases + [c for c in extra if (c.sub, c.cfg) == (sub, cfg)]
        n_a, n_b, at = sfc.layout(len(cases))
        h = session(sub, n_a, n_b, cfg, **more)
        xyz, step = sfc.build_records({at[i]: c.points for i, c in enumerate(cases)}, sub, n_a, n_b)
        words = records(xyz)
        what = "%s, %s" % (fam, cfg)
        got = h.device(words, step, k=K)
        exp = h.ref.process(xyz, step, None, K)
        same(got, exp, what)
        fitted = got["slope_a"] != sref.NOT_FITTED
        cells = [j * n_a + i for i, j in at[:len(cases)]]
        for c, cell in zip(cases, cells):
            assert got["count"][cell] == len(c.points), c.name
            value = dict(fitted=int(fitted[cell]), flat=int(got["flat"][cell]), level_q=int(got["level_q"][cell]), resid_q2=int(got["resid_q2"][cell]))
            for name, stated in c.expect.items():
                if name != "q_sign":
                    assert value[name] == stated, "%s: %s is %d on the device, stated %d (%s)" % (c.name, name, value[name], stated, c.edge)
            assert got["site"][cell] == got["flat"][cell], "a window of 0: a flat cell is a site"
            seen[c.name] = dict(value, site=int(got["site"][cell]), summary=got["summary"].tolist(), candidates=got["candidates"].tolist())
        empty = np.setdiff1d(np.arange(n_a * n_b), cells)
        assert not got["count"][empty].any() and np.all(got["level_q"][empty] == -(1 << 31)) and not got["flat"][empty].any()
        assert got["summary"].tolist() == [len(xyz), int(got["flat"].sum()), int(got["site"].sum()), int(fitted.sum())]
        assert int(fitted.sum()) == sum(int(fitted[cell]) for cell in cells)
        buf, cp, counts = shuffled_in_two_clouds(words, len(words))
        again = h.device(buf, step, cloud_points=cp, n_clouds=2, counts=counts, stride=cp, k=K)
        for o in OUT:
            assert again[o].tobytes() == got[o].tobytes() == np.asarray(exp[o]).astype(DTYPE[o]).tobytes(), "%s: %s, shuffled and in two clouds" % (what, o)
    return seen


def test_gate_cases_on_either_side_of_the_conditioning_gate():
    seen = run_family("gate")
    assert (seen["gate_one_off_holds"]["fitted"], seen["gate_one_off_fails"]["fitted"]) == (1, 0)
    assert (seen["gate_two_off_holds"]["fitted"], seen["gate_two_off_fails"]["fitted"]) == (1, 0)
    assert seen["gate_d_zero"]["fitted"] == 0 and seen["gate_a_zero"]["fitted"] == 0
    assert [seen["gate_count_%s" % n]["fitted"] for n in ("2_of_3", "3_of_3", "4_of_3", "6_of_7", "7_of_7", "8_of_7")] == [0, 1, 1, 0, 1, 1]
    assert seen["gate_one_off_holds"]["summary"][0] > 111000, "the whole cloud took part"


def test_gate_cases_in_a_session_of_one_block():
    """max_points 2,048: one block, whose LDS table takes all 18,643 (and 37,286) adds of a cell."""
    seen = run_family("gate", max_points=2048)
    assert all(h.slope.blocks == 1 for key, h in _made.items() if ("max_points", 2048) in key[4])
    assert [seen[n]["fitted"] for n in ("gate_one_off_holds", "gate_one_off_fails", "gate_two_off_holds", "gate_two_off_fails")] == [1, 0, 1, 0]


def test_tilt_cases_at_the_bound_move_the_sites_and_the_summary():
    seen = run_family("tilt")
    for axis in "uw":
        at, below, above = [seen["tilt_%s_%s" % (axis, tag)] for tag in ("at", "below", "above")]
        assert (at["flat"], below["flat"], above["flat"]) == (1, 0, 1) and (at["site"], below["site"], above["site"]) == (1, 0, 1)
    at, below = seen["tilt_u_at"], seen["tilt_u_below"]
    assert at["summary"][1:] == [2, 2, 2] and below["summary"][1:] == [0, 0, 2], "flat and sites fall, the fitted cells stay"
    assert at["candidates"][:2] != [NONE, NONE] and NONE not in at["candidates"][:2] and below["candidates"] == [NONE] * K
    lo, hi = seen["tilt_both_below"], seen["tilt_both_above"]
    assert (lo["flat"], hi["flat"]) == (0, 1) and lo["summary"][1:] == [0, 0, 1] and hi["summary"][1:] == [1, 1, 1]
    assert lo["candidates"][0] == NONE != hi["candidates"][0]


def test_resid_cases_at_the_bound_move_the_sites_and_the_summary():
    seen = run_family("resid")
    for d in (1, 25, 181):
        at, under = seen["resid_d%d_at" % d], seen["resid_d%d_under" % d]
        assert at["resid_q2"] == under["resid_q2"] == d * d and (at["flat"], under["flat"]) == (1, 0) and (at["site"], under["site"]) == (1, 0)
        assert at["summary"][1:3] == [1, 1] and under["summary"][1:3] == [0, 0] and under["summary"][3] == 1, "flat and sites fall, the cell stays fitted"
        assert at["candidates"][0] != NONE and under["candidates"] == [NONE] * K
    assert seen["resid_just_below"]["resid_q2"] == seen["resid_just_above"]["resid_q2"] == 627
    assert (seen["resid_just_below"]["flat"], seen["resid_just_above"]["flat"]) == (1, 0)
    wide = sfc.by_name("resid_wide").exact()
    assert seen["resid_wide"]["resid_q2"] == wide["resid_q2"] > 29000 ** 2 and seen["resid_wide"]["level_q"] == wide["level_q"]


def test_level_cases_round_the_tie_to_the_even_c0():
    seen = run_family("level", extra=[sfc.LOST])
    for tag, (c0, _, m, rc) in sfc.LEVEL_TIES.items():
        for name, shift in (("tie", 0), ("neg", -32000), ("negodd", -32001), ("pos", 32000)):
            assert seen["level_%s_%s" % (tag, name)]["level_q"] == m + shift + rc, (tag, name)
        assert seen["level_%s_down" % tag]["level_q"] <= seen["level_%s_tie" % tag]["level_q"] <= seen["level_%s_up" % tag]["level_q"]
    assert seen["lost_level_tie"]["level_q"] == 2, "the doubles' c0 lies just above -1.5 (exact least squares: 1)"


def test_thirds_cases_clamp_a_negative_q():
    seen = run_family("thirds")
    for c in sfc.family("thirds"):
        assert seen[c.name]["fitted"] == 1 and seen[c.name]["resid_q2"] == 0, c.name
        assert seen[c.name]["level_q"] == c.exact()["level_q"]


def test_noise_cases_are_the_reference_s_bytes():
    seen = run_family("noise")
    for c in sfc.family("noise"):
        e = c.exact()
        assert abs(seen[c.name]["level_q"] - e["level_q"]) <= 1 and abs(seen[c.name]["resid_q2"] - e["resid_q2"]) <= 1 and seen[c.name]["flat"] == int(e["flat"])
