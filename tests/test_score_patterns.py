"""What tests/score_patterns.py reaches, at the shapes and seeds tests/test_score_filter_values_gpu.py uses, and what
its patterns can tell apart: every slip of MUTANTS changes `out` or `grad` somewhere, each pattern kills the slips it was
built for, the one slip no input can show is proven so, and the restatement agrees with the exact-rational chain on a
crop of every pattern (tests/golden/score_filter.npz)."""
import os

import numpy as np
import pytest

import score_filter_ref as ref
import score_patterns as sp

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "score_filter.npz")
COMBOS = [(d, f) for d in (0, 1) for f in (4, 3)]
WHICH = ["camera", "ragged"]

# the slips each pattern was built to show
NAMED = {
    "planted_ties": ("a_half_up", "a_trunc"),
    "threshold_band": ("thr_1016", "thr_1018"),
    "b_extremes": ("other_t21", "b_trunc", "out_wrap", "out_sat254", "grad_sat"),
    "a_extremes": ("dir_swap",),
    "frame_vs_square": ("g13_about_square", "post_about_frame", "g13_border_reflect", "sobel_border_reflect",
                        "g21_border_reflect", "dir_swap"),
}


def _square_of(frame, sq):
    x, y, n = sq
    return frame[y:y + n, x:x + n].astype(np.int64)


def _killed(frame, sq, d, form, mutant, base=None):
    base = base or sp.stages_mutant(frame, sq, d, form)
    m = sp.stages_mutant(frame, sq, d, form, mutant)
    return bool((base["out"] != m["out"]).any()), bool((base["grad"] != m["grad"]).any())


@pytest.mark.parametrize("which", WHICH)
def test_restatement_without_a_slip_is_the_spec(which):
    for name in sp.PATTERNS:
        frame, sq = sp.pattern(name, which)
        for d, form in COMBOS:
            want, got = ref.stages(frame, sq, d, form), sp.stages_mutant(frame, sq, d, form)
            for key in ("A", "I", "M", "B", "out"):
                assert np.array_equal(got[key], want[key]), (name, d, form, key)
            o, g = ref.score_filter(frame, sq, d, form)
            assert np.array_equal(got["out"], o) and np.array_equal(got["grad"], g)


# ---- reach ---------------------------------------------------------------------------------------------------------
def _seam_class(u, tile, n):
    """0: within 13 after a tile seam (in the A halo of the tile before it), 1: within 13 before one, 2: neither."""
    d = u % tile
    return np.where((d < 13) & (u >= tile), 0, np.where((d >= tile - 13) & (u // tile < (n - 1) // tile), 1, 2))


@pytest.mark.parametrize("which", WHICH)
def test_planted_ties_reach(which):
    frame, sq = sp.pattern("planted_ties", which)
    n = sq[2]
    r, c, q = sp.tie_sites(frame, sq)
    odd = (q & 1) == 1
    print(which, "ties", len(r), "odd", int(odd.sum()), "even", int((~odd).sum()))
    assert len(r) >= (900 if which == "camera" else 120)
    assert abs(int(odd.sum()) - int((~odd).sum())) <= 0.05 * len(r)  # equal shares (random bytes: 5 ties, no odd q)
    # disjoint windows: any two ties at least 13 apart in one axis (chance ties aside: those share no grid point)
    on_grid = (r % sp.TIE_PITCH == 7) & (c % sp.TIE_PITCH == 7)
    assert on_grid.sum() >= 0.98 * len(r)
    for tile in (32, 64):  # ties on both sides of the seams and inside the tiles, along both axes
        for u in (r, c):
            cls = _seam_class(u[on_grid], tile, n)
            assert all((cls == k).sum() >= (100 if which == "camera" else 8) for k in range(3)), (tile, np.bincount(cls))
    for d in (0, 1):
        base = sp.stages_mutant(frame, sq, d, 4)
        for mutant, parity in (("a_half_up", 0), ("a_trunc", 1)):
            m = sp.stages_mutant(frame, sq, d, 4, mutant)
            dm = base["M"] != m["M"]
            if mutant == "a_half_up":  # half up and half to even part at the even ties alone
                da = np.argwhere(base["A"] != m["A"])
                assert {tuple(v) for v in da} == {(a, b) for a, b, qq in zip(r, c, q) if qq % 2 == 0}
            # a site counts when rounding ITS tie the other way moves an M inside the Sobel's reach of it
            eff = np.array([(qq & 1) == parity and dm[max(a - 3, 0):a + 4, max(b - 3, 0):b + 4].any() for a, b, qq in zip(r, c, q)])
            print(which, "direction", d, mutant, "sites that move an M:", int(eff.sum()))
            assert eff.sum() >= (150 if which == "camera" else 15)
            if which == "camera":  # ... on both sides of the seams of both tile sizes, along both axes
                for tile in (32, 64):
                    for u in (r, c):
                        cls = _seam_class(u, tile, n)
                        got = [int((eff & (cls == k)).sum()) for k in range(3)]
                        assert min(got) >= 10, (d, mutant, tile, got)  # (T = 32 leaves 6 of 32 columns to neither halo)
            if mutant == "a_half_up":  # and M moves `out` and `grad` (the sparse M keeps S + 2 B below 255)
                moved_out = np.array([(base["out"] != m["out"])[max(a - 10, 0):a + 11, max(b - 10, 0):b + 11].any() for a, b in zip(r, c)])
                assert (eff & moved_out).sum() >= 0.9 * eff.sum()
                assert (base["grad"] != m["grad"]).any()


@pytest.mark.parametrize("which", WHICH)
def test_threshold_band_reach(which):
    frame, sq = sp.pattern("threshold_band", which)
    for d in (0, 1):
        st = sp.stages_mutant(frame, sq, d, 4)
        counts = [int((st["I"] == v).sum()) for v in range(1015, 1019)]
        print(which, "direction", d, "pixels with I = 1015..1018:", counts, "Mfrac %.2f" % st["M"].mean())
        assert min(counts) >= (5 if which == "camera" else 2) and counts[1] >= 15 and counts[2] >= 100
        for form in (4, 3):  # the steep valleys hold a full window of ones: M = 1 regions wider than 21
            assert sp.stages_mutant(frame, sq, d, form)["B"].max() == sp.b_max(form)
        assert 0.1 < st["M"].mean() < 0.5


def test_b_max_comes_from_the_tap_sums():
    t4, t3 = ref.tap_tables(4)[1], ref.tap_tables(3)[1]
    assert (t4.sum(), t3.sum()) == (256, 254)
    assert sp.b_max(4) == 255 and sp.b_max(3) == 251 == (254 * 254 * 255) >> 16  # (remainder below one half)
    assert (254 * 254 * 255) & 0xFFFF < 0x8000


@pytest.mark.parametrize("which", WHICH)
def test_b_extremes_reach(which):
    frame, sq = sp.pattern("b_extremes", which)
    s = _square_of(frame, sq)
    for d, form in COMBOS:
        b = sp.stages_mutant(frame, sq, d, form)["B"]
        assert set(np.unique(b).tolist()) == set(range(sp.b_max(form) + 1)), (d, form)  # every value up to the maximum
        t = s + 2 * b
        small = [int(((t == v) & (s < 64)).sum()) for v in range(253, 258)]     # B of 95 and above on a low score
        large = [int(((t == v) & (s >= 128)).sum()) for v in range(253, 258)]
        print(which, d, form, "S + 2B = 253..257 with S < 64:", small, "with S >= 128:", large)
        assert min(small) >= 3 and min(large) >= 10, (d, form, small, large)
        assert (b >= 128).sum() > 1000 and ((b >= 100) & (b < 125)).any()  # the fusion rules' comparisons at 100 / 125


@pytest.mark.parametrize("which", WHICH)
def test_a_extremes_reach(which):
    frame, sq = sp.pattern("a_extremes", which)
    t13 = ref.tap_tables(4)[0]
    assert t13.sum() == 255 and (255 * 255 * 255 + 0x8000) >> 16 == 253
    for d in (0, 1):
        st = sp.stages_mutant(frame, sq, d, 4)
        h, p = sp.row_sums(frame, sq, d)
        print(which, "direction", d, "A", st["A"].min(), st["A"].max(), "H", h.min(), h.max(), "P", p.min(), p.max(),
              "I", st["I"].min(), st["I"].max())
        assert st["A"].min() == 0 and st["A"].max() == 253
        assert h.min() == 0 and h.max() == 255 * 255 == 65025 < 1 << 16         # the kernel's H buffer is uint16
        # ... and its P buffer int16: the bound is 253 * (sum of the row taps of one sign); the smoothing row of
        # direction 0 reaches it (a blurred A cannot follow the signs of the derivative row of direction 1)
        bound = 253 * (64 if d == 0 else 6)
        assert -(1 << 15) <= -bound <= p.min() and p.max() <= bound < 1 << 15
        assert d == 1 or p.max() == bound == 16192
        # |I| of both signs far beyond anything random bytes give (a few hundred), within 253 * 6 * 64
        assert st["I"].max() >= 6000 and st["I"].min() <= -6000 and np.abs(st["I"]).max() <= 253 * 6 * 64


@pytest.mark.parametrize("which", WHICH)
def test_frame_vs_square_reach(which):
    shape = sp.CAMERA[0] if which == "camera" else sp.RAGGED[0]
    for corner in ("tl", "br"):
        for inset in range(1, 7):
            frame, (x, y, n) = sp.frame_vs_square(shape, corner, inset)
            h, w = frame.shape
            assert 0 < x and 0 < y and x + n < w and y + n < h                      # strictly inside
            assert min(x, y, w - x - n, h - y - n) == inset                         # G13 reflects about the frame in part
            for d, form in (COMBOS if which == "ragged" else COMBOS[:1]):
                base = sp.stages_mutant(frame, (x, y, n), d, form)
                # (G13 reads 6 - inset rows past the frame's edge, with the taps 5, 9, 14 .. of 255: the kind of border
                # shows while it reads three rows or more, and at inset 6 it cannot show at all)
                for mutant in ("g13_about_square", "post_about_frame") + (("g13_border_reflect",) if inset <= 3 else ()):
                    assert any(_killed(frame, (x, y, n), d, form, mutant, base)), (corner, inset, d, form, mutant)


# ---- the kill matrix -----------------------------------------------------------------------------------------------
def test_kill_matrix(capsys):
    """Every slip changes out or grad on at least one pattern for every (direction, form); each pattern kills the slips
    named for it, at both shapes.  The printed matrix is the one in tests/README.md (X: all four (direction, form),
    else the number of them)."""
    rows = {}
    for name in sp.PATTERNS:
        frame, sq = sp.pattern(name, "ragged")
        base = {c: sp.stages_mutant(frame, sq, *c) for c in COMBOS}
        rows[name] = {m: [any(_killed(frame, sq, d, f, m, base[(d, f)])) for d, f in COMBOS] for m in sp.MUTANTS}
    with capsys.disabled():
        print("\n%-22s" % "slip" + "".join("%-17s" % n for n in sp.PATTERNS))
        for m in sp.MUTANTS:
            print("%-22s" % m + "".join("%-17s" % ("X" if all(rows[n][m]) else "." if not any(rows[n][m]) else sum(rows[n][m]))
                                        for n in sp.PATTERNS))
    for m in sp.MUTANTS:
        for k, c in enumerate(COMBOS):
            assert any(rows[n][m][k] for n in sp.PATTERNS), (m, c)
    for name, named in NAMED.items():
        for m in named:
            assert all(rows[name][m]), (name, m, rows[name][m])
    for name, named in NAMED.items():  # and at the camera shape
        frame, sq = sp.pattern(name, "camera")
        for d, f in COMBOS:
            base = sp.stages_mutant(frame, sq, d, f)
            for m in named:
                assert any(_killed(frame, sq, d, f, m, base)), (name, m, d, f)


def test_grad_sees_what_a_saturated_out_hides():
    """planted_ties with and without grad: both outputs change under the half-up slip, for every direction and form."""
    for which in WHICH:
        frame, sq = sp.pattern("planted_ties", which)
        for d, f in COMBOS:
            assert _killed(frame, sq, d, f, "a_half_up") == (True, True), (which, d, f)


def test_b_rounding_tie_cannot_be_killed():
    """B = round(255 s / 65536), s the G21 sum of a 0/1 image (s <= 256^2).  A tie needs 255 s = 32768 (mod 65536);
    255 is odd, hence invertible, so s = 32768 (mod 65536), and s <= 65536 leaves s = 32768 alone.  There the quotient
    127 is odd: half up and half to even both give 128.  So CV4 (half up) and CV3 (half to even) differ through
    their taps alone, and the slip `b_round_swap` changes no byte of any input: no pattern is built for it."""
    s = np.arange(256 * 256 + 1, dtype=np.int64)
    v = 255 * s
    ties = s[(v & 0xFFFF) == 0x8000]
    assert ties.tolist() == [32768] and ((255 * 32768) >> 16) == 127
    assert np.array_equal((v + 0x8000) >> 16, ref.rint_even_16(v))
    for name in sp.PATTERNS:  # ... and indeed
        frame, sq = sp.pattern(name, "ragged")
        for d, f in COMBOS:
            assert _killed(frame, sq, d, f, "b_round_swap") == (False, False)


# ---- the exact-rational chain ----------------------------------------------------------------------------------------
def test_pattern_crops_agree_with_the_exact_rational_chain():
    g = np.load(GOLDEN)
    names = [n for n in g["names"] if n.startswith("pat_")]
    crops = {name: (f, sq) for name, f, sq in sp.golden_crops()}
    assert sorted(names) == sorted(crops) and len(names) == 8
    fired = 0
    for name in names:
        frame, sq = crops[name]
        assert np.array_equal(g[f"{name}__frame"], frame) and tuple(g[f"{name}__square"]) == sq  # the stored crop IS the pattern's
        assert sq[2] <= 33
        for d, f in COMBOS:
            st = sp.stages_mutant(frame, sq, d, f)
            assert np.array_equal(st["A"], g[f"{name}__A"]), name
            assert np.array_equal(st["out"], g[f"{name}__d{d}_f{f}__out"]), (name, d, f)
            assert np.array_equal(st["grad"], g[f"{name}__d{d}_f{f}__grad"]), (name, d, f)
            fired += int(st["M"].any())
    assert fired >= 20
    # the crops keep what the patterns are about
    q = sp.tie_sites(*crops["pat_planted_ties"])[2]
    assert (q & 1).sum() >= 2 and ((q & 1) == 0).sum() >= 2
    for name, d in (("pat_threshold_band", 0), ("pat_threshold_band_t", 1)):
        i = sp.stages_mutant(*crops[name], d, 4)["I"]
        assert ((i == 1016).sum() or (i == 1018).sum()) and (i == 1017).sum() >= 10
    assert sp.stages_mutant(*crops["pat_b_extremes"], 0, 4)["B"].max() >= 250
    a = g["pat_a_extremes__A"]
    assert a.min() == 0 and a.max() == 253
