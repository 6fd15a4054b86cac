"""The built cells of tests/slope_fit_cases.py on the CPU: every case reaches the edge it names, in exact arithmetic and in
tests/sectors_slope_ref.py alike; SectorsSlopeRef.cells against exact least squares (Fractions) over every case, with the
measured worst differences asserted as they were measured; and the mutations of the fit, each killed by a named case.
tests/README_sectors_slope.md has the map and the measured figures.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import sectors_slope_ref as sref
import slope_fit_cases as sfc

F32 = np.float32
FIELDS = ("fitted", "slope_a", "slope_b", "level_q", "resid_q2", "flat")
_ref, _copy = {}, {}


def ref_cell(c):
    """SectorsSlopeRef.cells of the case's points, alone in cell 0 -> its outputs as Python integers (the slopes as bits)."""
    if c.name not in _ref:
        p = np.asarray(c.points, dtype=np.int64)
        out = sfc.ref_of(sub=c.sub, **c.cfg).cells(np.zeros(len(p), dtype=np.int64), p[:, 2], p[:, 0], p[:, 1])
        _ref[c.name] = {f: int(out[f][0]) for f in FIELDS}
    return _ref[c.name]


def copy_cell(c, ops=None):
    if ops is not None:
        return sfc.fit_copy(c.points, sub=c.sub, ops=ops, **c.cfg)
    if c.name not in _copy:
        _copy[c.name] = sfc.fit_copy(c.points, sub=c.sub, **c.cfg)
    return _copy[c.name]


def as_f32(bits):
    return np.array([bits], dtype=np.uint32).view(F32)[0]


# ------------------------------------------------------------------------------------------------ the oracle and the builder
def test_the_oracle_by_hand_and_the_builder_places_records():
    """k = 5 + 3 u - 2 w on four corners: the plane itself; one height moved: by hand.  nearest_float32 and round_half_even
    at their ties.  The builder refuses a record that does not land in its cell."""
    e = sfc.exact_fit([(-7, -7, 5 - 21 + 14), (7, -7, 5 + 21 + 14), (-7, 7, 5 - 21 - 14), (7, 7, 5 + 21 - 14)], min_count=4)
    assert (e["c"], e["gu"], e["gw"], e["rss"], e["one_minus_rho2"], e["fitted"]) == (5, 3, -2, 0, 1, True)
    assert e["slope_a"] == F32(0.1875) and e["slope_b"] == F32(-0.125) and e["level_q"] == 5 and e["resid_q2"] == 0 and e["flat"]
    assert not sfc.exact_fit([(-7, -7, 0), (7, -7, 0), (-7, 7, 0), (7, 7, 0)], min_count=5)["fitted"]
    # (-1, 0), (1, 0), (0, 1) in units of 7 ... by hand on three points and a fourth off the plane by 4: every residual is +-1
    e = sfc.exact_fit([(-7, -7, 0), (7, -7, 0), (-7, 7, 0), (7, 7, 4)])
    assert (e["c"], e["gu"], e["gw"], e["rss"]) == (1, Fraction(1, 7), Fraction(1, 7), 4) and e["resid_q2"] == 1
    assert [sfc.round_half_even(Fraction(n, 2)) for n in (-5, -3, -1, 1, 3, 5, 4)] == [-2, -2, 0, 0, 2, 2, 2]
    assert sfc.nearest_float32(Fraction(1, 3)) == F32(1.0 / 3.0) and sfc.nearest_float32(Fraction(-3, 16)) == F32(-0.1875)
    tie = Fraction(1) + Fraction(1, 1 << 24)                       # half-way between 1 and the next float32: to even
    assert sfc.nearest_float32(tie) == F32(1.0) and sfc.nearest_float32(tie + Fraction(1, 1 << 23)) == F32(1.0) + F32(2.0 ** -22)
    assert sfc.ulps(F32(1.0), np.nextafter(F32(1.0), F32(2))) == 1 and sfc.ulps(F32(0.0), F32(-0.0)) == 0
    assert sfc.ulps(np.nextafter(F32(0), F32(1)), np.nextafter(F32(0), F32(-1))) == 2
    xyz, step = sfc.build_records({(1, 2): [(-7, 7, 3)], (3, 0): [(1, -1, -2)]}, 8, 4, 3, origin=(4.0, -2.5, 1.25))
    assert xyz.tolist() == [[4.0 + 0.5 + 0.03125, -2.5 + 1.0 + 0.46875, 1.25 + 3 / 512], [4.0 + 1.5 + 0.28125, -2.5 + 0.21875, 1.25 - 2 / 512]]
    with pytest.raises(AssertionError):
        sfc.build_records({(0, 0): [(-7, 7, 40000)]}, 8, 4, 3)      # |k| > 32,767 takes no part
    with pytest.raises(AssertionError):
        sfc.build_records({(0, 0): [(1, 1, 1)]}, 8, 4, 3, origin=(0.1, 0.0, 0.0))


def test_the_copy_of_the_fit_is_the_reference():
    """fit_copy with its own operators gives SectorsSlopeRef.cells' words on every case: what the mutations depart from."""
    for c in sfc.CASES:
        got, want = copy_cell(c), ref_cell(c)
        assert {f: got[f] & 0xFFFFFFFF for f in FIELDS} == {f: want[f] & 0xFFFFFFFF for f in FIELDS}, c.name


# ------------------------------------------------------------------------------------------------ every case reaches its edge
def test_every_case_states_its_decisions_and_both_hold_them():
    assert {c.family for c in sfc.CASES} == set(sfc.FAMILIES) and all(c.edge and c.expect for c in sfc.CASES)
    for c in sfc.CASES:
        e, r = c.exact(), ref_cell(c)
        for what, value in c.expect.items():
            if what == "q_sign":
                continue
            assert int(e[what]) == value, (c.name, what, "exact")
            assert r[what] == value, (c.name, what, "reference")


def test_gate_cases_straddle_the_threshold_and_double_agrees():
    for holds, fails in (("gate_one_off_holds", "gate_one_off_fails"), ("gate_two_off_holds", "gate_two_off_fails")):
        h, f = sfc.by_name(holds).exact(), sfc.by_name(fails).exact()
        assert h["enough"] and f["enough"] and h["gate"] and not f["gate"]
        assert f["one_minus_rho2"] < Fraction(1, 1 << 20) < h["one_minus_rho2"] < Fraction(1001, 1000 << 20), "within a part in a thousand"
        assert f["n"] - h["n"] == 2, "neighbouring counts"
        assert h["AC"] > 1 << 53, "A C rounds in double"
    assert sfc.by_name("gate_one_off_holds").exact()["n"] == 18641 and sfc.by_name("gate_one_off_fails").exact()["n"] == 18643
    for c in sfc.family("gate"):             # each is about the gate, not about rounding: double and exact integers agree
        assert ref_cell(c)["fitted"] == int(c.exact()["fitted"]), c.name
        assert any(k != 0 for _, _, k in c.points)
    d0, a0 = sfc.by_name("gate_d_zero").exact(), sfc.by_name("gate_a_zero").exact()
    assert d0["AC"] > 0 and d0["D"] == 0 and d0["enough"] and len({u for u, _, _ in sfc.by_name("gate_d_zero").points}) > 3
    assert a0["AC"] == 0 and a0["enough"] and len({u for u, _, _ in sfc.by_name("gate_a_zero").points}) == 1
    assert len({w for _, w, _ in sfc.by_name("gate_a_zero").points}) > 1, "C > 0"
    for min_count, names in ((1, ("gate_count_2_of_3", "gate_count_3_of_3", "gate_count_4_of_3")), (7, ("gate_count_6_of_7", "gate_count_7_of_7", "gate_count_8_of_7"))):
        cs = [sfc.by_name(n) for n in names]
        min_fit = max(min_count, 3)
        assert [c.exact()["n"] for c in cs] == [min_fit - 1, min_fit, min_fit + 1] and all(c.cfg["min_count"] == min_count for c in cs)
        assert [c.exact()["gate"] for c in cs[1:]] == [True, True] and [c.exact()["fitted"] for c in cs] == [False, True, True]
    assert sfc.by_name("gate_count_6_of_7").exact()["gate"], "six points that the gate would pass: the count refuses them"


def test_tilt_cases_sit_on_the_bound():
    at = Fraction(float(F32(0.1875))) ** 2
    for axis in "uw":
        cs = [sfc.by_name("tilt_%s_%s" % (axis, tag)) for tag in ("below", "at", "above")]
        for c in cs:
            e = c.exact()
            assert e["tilt2"] == at and e["rss"] == 0 and (e["gu"], e["gw"]) == ((3, 0) if axis == "u" else (0, -3))
        ms = [np.float32(c.cfg["max_slope"]) for c in cs]
        assert ms[1] == F32(0.1875) and ms[0] == np.nextafter(ms[1], F32(0)) and ms[2] == np.nextafter(ms[1], F32(1))
        assert [c.exact()["tilt_ok"] for c in cs] == [False, True, True] and all(c.exact()["resid_ok"] for c in cs)
    lo, hi = sfc.by_name("tilt_both_below"), sfc.by_name("tilt_both_above")
    assert lo.points == hi.points and lo.exact()["tilt2"] == Fraction(5, 36) and lo.exact()["gu"] != 0 != lo.exact()["gw"] and lo.exact()["rss"] == 0
    assert np.float32(hi.cfg["max_slope"]) == np.nextafter(np.float32(lo.cfg["max_slope"]), F32(1)), "neighbouring float32"
    assert Fraction(lo.cfg["max_slope"]) ** 2 < Fraction(5, 36) < Fraction(hi.cfg["max_slope"]) ** 2
    f = copy_cell(lo)
    sa, sb = float(as_f32(f["slope_a"])), float(as_f32(f["slope_b"]))
    assert Fraction(5, 36).denominator & (Fraction(5, 36).denominator - 1), "5/36 is no double: the sum rounds"
    assert abs(sa * sa + sb * sb - 5.0 / 36.0) < 1e-7
    assert (lo.exact()["tilt_ok"], hi.exact()["tilt_ok"]) == (False, True) and (ref_cell(lo)["flat"], ref_cell(hi)["flat"]) == (0, 1)


def test_resid_cases_sit_on_the_bound():
    for d in (1, 25, 181):
        at, under = sfc.by_name("resid_d%d_at" % d), sfc.by_name("resid_d%d_under" % d)
        e = at.exact()
        assert at.points == under.points and e["rss"] == d * d * e["n"] and (e["gu"], e["gw"], e["c"]) == (3, -2, 40)
        assert (at.cfg["max_spread_q2"], under.cfg["max_spread_q2"]) == (d * d, d * d - 1) and at.exact()["tilt_ok"] and under.exact()["tilt_ok"]
        assert (at.exact()["resid_ok"], under.exact()["resid_ok"]) == (True, False)
    below, above = sfc.by_name("resid_just_below").exact(), sfc.by_name("resid_just_above").exact()
    assert below["rss"] / below["n"] == 628 - Fraction(6363, 3024236) and above["rss"] / above["n"] == 627 + Fraction(23, 27311)
    assert below["resid_q2"] == above["resid_q2"] == 627 and below["tilt_ok"] and above["tilt_ok"]
    wide = sfc.by_name("resid_wide")
    e, ks = wide.exact(), [k for _, _, k in wide.points]
    S = sum((k - e["m"]) ** 2 for k in ks)
    assert e["n"] * S > 1 << 53 and max(ks) > 32000 and min(ks) < -32000 and e["su"] != 0 and e["sw"] != 0
    assert e["gu"].denominator & (e["gu"].denominator - 1), "gu is no double"
    frac = e["rss"] / e["n"] - e["resid_q2"]
    assert Fraction(1, 1000) < frac < Fraction(999, 1000), "RSS / N far from an integer: the floor is rounding-proof"


def test_level_cases_are_ties_in_exact_arithmetic():
    rounded = {Fraction(-3, 2): -2, Fraction(-1, 2): 0, Fraction(1, 2): 0, Fraction(3, 2): 2, Fraction(5, 2): 2}
    assert sorted(t[0] for t in sfc.LEVEL_TIES.values()) == sorted(rounded)
    odd_m = not_whole = 0
    for tag, (c0, pts, m, rc) in sfc.LEVEL_TIES.items():
        assert rc == rounded[c0] and len(pts) <= 8 and all(abs(u) <= 3 and abs(w) <= 3 for u, w, _ in pts)
        for name, shift in (("tie", 0), ("neg", -32000), ("negodd", -32001), ("pos", 32000)):
            c = sfc.by_name("level_%s_%s" % (tag, name))
            e = c.exact()
            assert e["c0"] == c0 and e["m"] == m + shift and e["su"] != 0 and e["level_q"] == m + shift + rc, c.name
            odd_m += e["m"] % 2
            if e["m"] % 2:
                assert e["level_centre"] != e["level_q"], "an odd m: the tie goes to the even c0, which is the odd level"
            else:
                assert e["level_centre"] == e["level_q"]
            if shift < 0:
                ks = [k for _, _, k in c.points]
                assert max(ks) < 0 and sum(ks) % len(ks) == sum(k for _, _, k in pts) % len(ks)
                if sum(ks) % len(ks):
                    assert sfc.trunc_mean(sum(ks), len(ks)) == e["m"] + 1, "the floor mean is not the truncated mean"
                    not_whole += 1
        down, up = sfc.by_name("level_%s_down" % tag).exact(), sfc.by_name("level_%s_up" % tag).exact()
        assert down["c"] < m + c0 < up["c"] and down["level_q"] <= up["level_q"]
        assert sum(abs(a[2] - b[2]) for a, b in zip(sfc.by_name("level_%s_down" % tag).points, pts)) == 1
    assert odd_m >= 5 and not_whole >= 6
    # a tie in exact arithmetic that the doubles lose: the computed c0 is not -1.5, and level_q is a quantum off
    lost = sfc.LOST
    e, f = lost.exact(), copy_cell(lost)
    assert e["c0"] == Fraction(-3, 2) and e["level_q"] == 1 and -1.5 < f["c0"] < -1.5 + 1e-14 and f["level_q"] == ref_cell(lost)["level_q"] == 2


def test_thirds_cases_hold_both_signs_of_q():
    signs = set()
    for c in sfc.family("thirds"):
        e, f = c.exact(), copy_cell(c)
        assert e["rss"] == 0 and e["gu"].denominator == 3 and e["gw"] == 2 * e["gu"], c.name
        sign = "negative" if f["Q"] < 0 else "positive" if f["Q"] > 0 else "zero"
        assert sign == c.expect["q_sign"] and f["resid_q2"] == 0, c.name
        signs.add(sign)
    assert signs == {"negative", "positive", "zero"} and len(sfc.family("thirds")) == 9
    found, counts = sfc.search_thirds()
    assert found == sfc.THIRDS and counts["negative"] >= 40 and counts["positive"] >= 40, "the literal lists are the seeded search's"


def test_noise_cases_are_what_the_issue_lists():
    cs = sfc.family("noise")
    assert sorted((c.sub, len(c.points)) for c in cs) == [(s, n) for s in (2, 8, 16) for n in (3, 17, 64, 1025)]
    for c in cs:
        e = c.exact()
        assert e["fitted"] and (e["su"] != 0 or e["sw"] != 0) and e["tilt2"] < 0.85 ** 2
        if len(c.points) >= 17:
            assert e["rss"] > 0


# ------------------------------------------------------------------------------------------------ against exact least squares
# measured once, then asserted as measured: both sides are deterministic CPU arithmetic (tests/README_sectors_slope.md)
MEASURED = dict(slope_ulps=0, level_quanta=1, resid_quanta2=0, cells_not_equal=1, cells=81)      # (the one: lost_level_tie)


def test_the_reference_against_exact_least_squares():
    every = sfc.CASES + [sfc.LOST]
    worst = dict(slope_ulps=0, level_quanta=0, resid_quanta2=0, cells_not_equal=0, cells=len(every))
    for c in every:
        e, r, f = c.exact(), ref_cell(c), copy_cell(c)
        assert r["fitted"] == int(e["fitted"]) and r["flat"] == int(e["flat"]), c.name
        d_level, d_resid, d_slope = abs(r["level_q"] - e["level_q"]), abs(r["resid_q2"] - e["resid_q2"]), 0
        if e["fitted"]:
            # the tilt and the residual decision, each alone (the copy is the reference: test_the_copy_of_the_fit_is_the_reference)
            assert (r["resid_q2"] <= c.cfg["max_spread_q2"]) == e["resid_ok"], c.name
            sa, sb = float(f["sa"]), float(f["sb"])
            assert (sa * sa + sb * sb <= sref.max_tilt2_of(c.cfg["max_slope"])) == e["tilt_ok"], c.name
            d_slope = max(sfc.ulps(as_f32(r["slope_a"]), e["slope_a"]), sfc.ulps(as_f32(r["slope_b"]), e["slope_b"]))
            if e["one_minus_rho2"] >= Fraction(1, 1 << 10):
                assert d_slope <= 1, (c.name, d_slope)
        else:
            assert r["slope_a"] == r["slope_b"] == sref.NOT_FITTED
        assert d_level <= 1 and d_resid <= 1, (c.name, d_level, d_resid)
        exact_family = c.family in ("tilt", "level") or (c.family == "resid" and "just" not in c.name)
        if exact_family:
            assert (d_slope, d_level, d_resid) == (0, 0, 0), c.name
        worst["slope_ulps"], worst["level_quanta"] = max(worst["slope_ulps"], d_slope), max(worst["level_quanta"], d_level)
        worst["resid_quanta2"] = max(worst["resid_quanta2"], d_resid)
        worst["cells_not_equal"] += (d_slope, d_level, d_resid) != (0, 0, 0)
        if (d_slope, d_level, d_resid) != (0, 0, 0):
            print("not equal: %s: %d ulps, level %d, resid %d" % (c.name, d_slope, d_level, d_resid))
    print("measured:", worst)
    assert worst == MEASURED


# ------------------------------------------------------------------------------------------------ mutations of the formula
# the gate's > and >= part only where D 2^20 == A C: in exact integers A C - B B == A C / 2^20, that is B B == (2^20 - 1) g and
# A C == 2^20 g with g = 41,943 t^2 (2^20 - 1 = 3 * 5^2 * 11 * 31 * 41); no cell built here has it, and no test can tell the two
EQUIVALENT_HERE = ("gate >= for >",)
KILLERS = {
    "tilt < for <=": ("tilt_u_at", "tilt_w_at"),
    "resid < for <=": ("resid_d1_at", "resid_d25_at", "resid_d181_at"),
    "count > for >=": ("gate_count_3_of_3", "gate_count_7_of_7"),
    "B with the wrong sign": ("gate_one_off_holds", "gate_two_off_holds", "tilt_both_above", "resid_wide"),
    "trunc for rint": ("level_m1p5_tie", "level_p1p5_tie", "level_p1p5_negodd"),
    "half up for half to even": ("level_m1p5_tie", "level_p0p5_tie", "level_p2p5_tie", "level_p0p5_negodd"),
    "the clamp of Q dropped": ("thirds_negative_0", "thirds_negative_1", "thirds_negative_2"),
    "the truncated mean for the floor mean": ("level_m0p5_neg", "level_p0p5_negodd"),
    "gu and gw exchanged": ("tilt_u_at", "tilt_w_at", "resid_d25_at"),
    "scale without the factor 2P": ("tilt_u_at", "tilt_both_above", "noise_sub2_n17"),
    "suk', swk' without m": ("level_p0p5_tie", "resid_wide", "noise_sub16_n1025"),
}


@pytest.mark.parametrize("name", list(sfc.MUTATIONS))
def test_each_mutation_of_the_fit_is_killed_by_a_named_case(name):
    killed = []
    for c in sfc.CASES:
        got, want = copy_cell(c, sfc.MUTATIONS[name]), copy_cell(c)
        if any(got[f] != want[f] for f in FIELDS):
            killed.append(c.name)
    print("%s: killed by %d cases: %s" % (name, len(killed), ", ".join(killed[:8])))
    if name in EQUIVALENT_HERE:
        assert not killed, "a case now reaches D 2^20 == A C: take the mutation off EQUIVALENT_HERE"
        return
    assert killed, "no case kills it"
    assert set(KILLERS[name]) <= set(killed), "the cases built for this edge"
