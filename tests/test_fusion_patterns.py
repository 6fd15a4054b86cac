"""tests/fusion_patterns.py without a GPU: each generator reaches what it was built to reach at exactly the cases
test_fusion_values_gpu.py runs, rules_ref and the restated kernel agree with the oracle on every pattern, and the kill
matrix of tests/README.md ("Fusion patterns") holds: which slip of the restated kernel which generator shows."""
import functools

import numpy as np
import pytest

import oracle
import fusion_patterns as fp
import test_fusion_values_gpu as gpu

GEOMETRY = gpu.GEOMETRY


def test_the_case_list_is_the_gpu_file_s():
    """Any other case list is refused: the reach below is asserted for what runs on the device, nothing else."""
    assert len(GEOMETRY) == 123 and [c["name"] for c in GEOMETRY].count("size") == len(gpu.WIDTHS) * len(gpu.HEIGHTS)
    assert gpu.WIDTHS == (1, 2, 3, 4, 5, 7, 8, 247, 248, 249, 251, 252, 496, 497) and gpu.HEIGHTS == (1, 2, 3, 4, 5, 7)
    assert gpu.FUSE_ROWS == (0, 2, 4, 6, 16)
    assert sorted({(c["h"], c["rows"]) for c in GEOMETRY if c["name"] == "fuse_rows"}) == sorted(
        {(h, r) for r in gpu.FUSE_ROWS for h in (r - 1, r, r + 1, 2 * r + 1, 4 * r + 2) if h >= 1})
    crops = [c["crop"] for c in GEOMETRY if c["name"] == "crop"]
    assert {l % 4 for l, _, _, _ in crops} == {0, 1, 2, 3} and gpu.REFERENCE_CROP in crops
    sizes = [(c["h"] - c["crop"][2] - c["crop"][3], c["w"] - c["crop"][0] - c["crop"][1]) for c in GEOMETRY if c["name"] == "crop"]
    assert any(w == 1 and h > 1 for h, w in sizes) and any(h == 1 and w > 1 for h, w in sizes) and (1, 1) in sizes
    lay = [c for c in GEOMETRY if c["layout"]]
    assert all(c["frames"] == 3 and len(set(c["layout"][0])) == 6 and set(c["layout"][1]) == {0, 1, 2, 3} and c["layout"][2]
               for c in lay) and any(c["w"] < 4 for c in lay)
    six = [c for c in GEOMETRY if c["name"] == "six_strips"]
    assert [(c["w"], c["h"], c["frames"]) for c in six] == [(1241, 5, 2)] and -(-1241 // fp.STRIP) == 6
    assert gpu.TABLE_CASES == [(r, c) for r in fp.RULES for c in (True, False)]
    assert gpu.NODE_SEAMS == dict(seams_x=(63, 64, 127, 128), seams_y=(15, 16, 63, 64)) and gpu.NODE_TALL == (736, 16)
    assert [n for n, _ in gpu.NODE_CASES] == [192] * 3 and {c[0] for _, c in gpu.NODE_CASES} == {0, 64, 63}


# ---- what is cached: tables, frames, the oracle's answers -------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _table(rule):
    out = []
    for name, planes in fp.rule_table(rule):
        six = planes + [planes[2], planes[1]]
        out.append((name, six, oracle.fuse(six, rule=rule, crop=(0, 0, 0, 0))))
    return out


def _geo(case, frames):
    return dict(crop=case["crop"], combined=case["combined"],
                rows=fp.rows_per_wave(case["w"], case["h"], frames, case["combined"], case["rows"]))


@functools.lru_cache(maxsize=None)
def _frames(rule, k, which):
    """[(six planes of one frame, the oracle's answer in the model's form)], geometry"""
    case = GEOMETRY[k]
    planes = gpu.lively_planes(rule, case, k) if which == "lively" else gpu.edge_planes(rule, case)
    if case["layout"] and case["layout"][2]:
        planes[4] = planes[2]
    out = []
    for f in range(planes[0].shape[0]):
        six = [np.ascontiguousarray(p[f]) for p in planes]
        out.append((six, fp.expected_as_model(*oracle.fuse(six, rule=rule, crop=case["crop"], want_combined=case["combined"]))))
    return out, _geo(case, len(out))


def _edge_rule(k):
    return fp.PASS_THROUGH[k % len(fp.PASS_THROUGH)]


SEAMS_K = next(k for k, c in enumerate(GEOMETRY) if c["name"] == "seams")


def _patterns():
    """(rule, k, which) of every lively case of every rule and of the median_edges cases under one rule each (the plane
    the median sees is the same under all eight; the `seams` case runs all eight)."""
    for k, case in enumerate(GEOMETRY):
        for rule in fp.RULES:
            yield rule, k, "lively"
        if case["edges"]:
            for rule in (fp.PASS_THROUGH if k == SEAMS_K else (_edge_rule(k),)):
                yield rule, k, "edges"


# ---- reach ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule", fp.RULES)
def test_rule_table_reaches_every_class_lane_and_comparison(rule):
    S, D = fp.score_edges(rule), fp.D_EDGE
    assert {0, 255} <= set(S) and all({t - 1, t, t + 1} <= set(S) for t in fp.THRESHOLDS[rule])
    assert {0, 1, 229, 230, 231, 254, 255} <= set(D)
    tables = _table(rule)
    names = [n for n, _, _ in tables]
    assert names[:2] == ["edges", "edges_narrow"] and len(names) == 2 + len(fp.FULL_TABLE_SCORES[rule])
    edges = tables[0][1]
    assert edges[0].shape[0] == 3 * len(S) * len(D) and all(max(p[0].shape) <= 768 for n, p, _ in tables if n != "edges_narrow")
    cells = [p[1::3, 1::3] for p in edges[:4]]
    assert np.array_equal(np.repeat(np.repeat(cells[0], 3, 0), 3, 1), edges[0])  # 3 x 3 cells, constant
    assert len({tuple(v) for v in np.stack([c.ravel() for c in cells], 1).tolist()}) == (len(S) * len(D)) ** 2
    narrow = tables[1][1]
    assert narrow[0].shape == (3 * cells[0].size, 3) and all(np.array_equal(n[1::3, 1], c.ravel()) for n, c in zip(narrow, cells))
    # every outcome class in every byte lane (x mod 4: dword of even / odd pixels, low / high field), in both kernels
    for planes, lanes in ((edges, 4), (narrow, 3)):
        cls = fp.outcome_class(rule, *planes[:4])
        x = np.broadcast_to(np.arange(cls.shape[1]) % 4, cls.shape)
        for c in range(len(fp.CLASSES[rule])):
            assert set(np.unique(x[cls == c])) == set(range(lanes)), (fp.CLASSES[rule][c], lanes)
    # one whole table of 65,536 distance pairs per class whose output depends on them
    for (name, six, _), pair in zip(tables[2:], fp.FULL_TABLE_SCORES[rule]):
        a, b = (six[2], six[3]) if pair == "scores" else (six[0], six[1])
        assert len(set(zip(a[1::3, 1::3].ravel().tolist(), b[1::3, 1::3].ravel().tolist()))) == 65536
    full_classes = {int(c) for _, six, _ in tables[2:] for c in np.unique(fp.outcome_class(rule, *six[:4]))}
    depends = {fp.WEIGHTED_AVERAGE: {0, 1, 2}, fp.MAX_DIST: {0, 1, 2}, fp.MAX_DIST_UNLESS_BLACK: {0, 1}, fp.BETTER_SCORE: {0, 1},
               fp.ONLY_GOOD_1: {0}, fp.ONLY_GOOD_AVG: {0}, fp.OVERLAP: set(), fp.BLACK_TO_WHITE: {0}, fp.GRAD_FILTER: {0, 1, 2}}
    assert depends[rule] <= full_classes
    # every comparison of the rule's code sees a - b = -1, 0, +1 and, where bytes allow it, |a - b| >= 128 in both signs
    d1, d2, s1, s2 = (c.astype(np.int64) for c in cells)
    k = lambda v: np.int64(v)  # noqa: E731
    comparisons = {fp.WEIGHTED_AVERAGE: [(s1, k(1)), (s2, k(1))], fp.MAX_DIST: [(d1, d2)],
                   fp.MAX_DIST_UNLESS_BLACK: [(d1, k(1)), (d2, k(1))], fp.BETTER_SCORE: [(s1, s2)], fp.ONLY_GOOD_1: [(s2, k(50))],
                   fp.ONLY_GOOD_AVG: [(s1, k(100)), (s2, k(100))], fp.OVERLAP: [(s1, s2), (s2, s1), (s1, k(20)), (s2, k(20))],
                   fp.BLACK_TO_WHITE: [],
                   fp.GRAD_FILTER: [(s1, s2), (s2, s1), (s1, k(100)), (s2, k(100)), (d1, k(230)), (d2, k(230)), (s1, k(125)),
                                    (s2, k(125)), (5 * d1, 4 * d2), (4 * d1, 5 * d2)]}[rule]
    for a, b in comparisons:
        diff = set(np.unique(a - b).tolist())
        assert {-1, 0, 1} <= diff, (rule, diff)
        if b.ndim:  # two bytes: both signs; a byte against a constant c: a - c >= 128 needs c <= 127, <= -128 needs c >= 128
            assert min(diff) <= -128 and max(diff) >= 128
        else:
            assert (max(diff) >= 128) if b <= 127 else (min(diff) <= -128)


def test_lively_shares_and_distinct_values():
    """Asserted, not measured: every outcome class holds a tenth of the pixels or more (from 8 pixels on; below that the
    classes differ by one pixel at most), and the fused image takes 64 distinct values (a value per 16 pixels on the small
    shapes) where the rule can produce that many -- OVERLAP: all three from 48 pixels on."""
    for k, case in enumerate(GEOMETRY):
        for rule in fp.RULES:
            frames, _ = _frames(rule, k, "lively")
            for six, (fused, _) in frames:
                n, ncls = six[0].size, len(fp.CLASSES[rule])
                counts = np.bincount(fp.outcome_class(rule, *six[:4]).ravel(), minlength=ncls)
                assert counts.max() - counts.min() <= 1, (rule, k)
                if n >= 8:
                    assert (10 * counts >= n).all(), (rule, k, counts)
                if case["crop"] == (0, 0, 0, 0):
                    distinct = len(np.unique(fused))
                    if rule == fp.OVERLAP:
                        assert distinct == 3 or n < 48, (k, n, distinct)
                    else:
                        assert distinct >= min(64, n // 16), (rule, k, n, distinct)


def test_median_edges_reach_every_window_count_lane_and_border():
    for (h, w, kw) in [(GEOMETRY[SEAMS_K]["h"], GEOMETRY[SEAMS_K]["w"], {})] + [(n, n, gpu.NODE_SEAMS) for n in (192, 736)]:
        frames, where = fp.edge_frames(h, w, **kw)
        seams = kw.get("seams_x", (247, 248, 495, 496))
        high = frames == frames.max()
        for x in seams:  # windows of exactly c = 0..9 high pixels centred on each seam column
            for c in range(10):
                f, y = where[(x, c)]
                assert high[f, y - 1:y + 2, x - 1:x + 2].sum() == c, (x, c)
        # single pixels: alone in their 5 x 5 surround, bright on dark and dark on bright, at every x mod 4 beside ...
        for level, name in ((True, "bright"), (False, "dark")):
            pad = np.pad(high, ((0, 0), (2, 2), (2, 2)), mode="constant", constant_values=not level)
            alone = np.zeros_like(high)
            for f in range(fp.FIXED, len(frames)):
                is_l = pad[f] == level
                count = sum(is_l[dy:dy + h, dx:dx + w] for dy in range(5) for dx in range(5))
                alone[f] = (high[f] == level) & (count == 1)
            ys, xs = np.nonzero(alone.any(axis=0))
            at = set(zip(ys.tolist(), xs.tolist()))
            cols = set(range(4)) | set(range(w - 4, w)) | {s + d for s in seams for d in range(-3, 5) if s + d < w}
            rows = {0, 1, h - 2, h - 1} | {y for y in kw.get("seams_y", (3, 4, 7, 8, 15, 16)) if y < h}
            assert {(y, x) for y in rows for x in cols} <= at, name
            assert {(0, 0), (0, w - 1), (h - 1, 0), (h - 1, w - 1)} <= at
    # every geometry case: stripes of period 2, 3, 4 both ways and the checkerboard come first; values stay pass-through
    for k, case in enumerate(GEOMETRY):
        if case["edges"]:
            fr, _ = fp.edge_frames(case["h"], case["w"])
            assert len(fr) >= fp.FIXED and set(np.unique(fr)) <= {7, 201}
            yy, xx = np.mgrid[0:case["h"], 0:case["w"]]
            for f, mask in enumerate([xx % 2 == 0, xx % 3 == 0, xx % 4 == 0, yy % 2 == 0, yy % 3 == 0, yy % 4 == 0, (xx + yy) % 2 == 0]):
                assert np.array_equal(fr[f] == 201, mask)


# ---- references -------------------------------------------------------------------------------------------------------
def test_rules_ref_equals_the_oracle_on_every_pattern_and_cell():
    for rule in fp.RULES:
        for name, six, want in _table(rule):
            got = fp.fuse_ref(rule, six)
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (rule, name)
            if name != "edges_narrow":  # (the same cells once more)
                cells = np.stack([p[1::3, 1::3].ravel() for p in six[:4]], 1).astype(np.int64)
                ref = fp.rules_ref(rule, *cells.T)
                pix = np.fromiter((oracle.fuse_pixel(rule, *row) for row in cells.tolist()), dtype=np.int64, count=len(cells))
                assert np.array_equal(pix & 0xFF, ref), (rule, name)
    for rule, k, which in _patterns():
        case = GEOMETRY[k]
        for six, want in _frames(rule, k, which)[0]:
            got = fp.expected_as_model(*fp.fuse_ref(rule, six, case["crop"], case["combined"]))
            assert fp.same(got, want), (rule, k, which)


def test_the_model_without_a_slip_equals_the_oracle_on_every_pattern():
    for rule in fp.RULES:
        for name, six, want in _table(rule):
            geo = dict(crop=(0, 0, 0, 0), combined=True, rows=fp.rows_per_wave(six[0].shape[1], six[0].shape[0], 1, True))
            assert fp.same(fp.fuse_model(rule, six, geo), fp.expected_as_model(*want)), (rule, name)
    for rule, k, which in _patterns():
        frames, geo = _frames(rule, k, which)
        for six, want in frames:
            assert fp.same(fp.fuse_model(rule, six, geo), want), (rule, k, which)


def test_rows_per_wave_is_launch_fuse_s_choice():
    assert fp.rows_per_wave(2160, 2160, 3, True) == 8 and fp.rows_per_wave(2160, 2160, 3, False) == 16
    assert fp.rows_per_wave(768, 768, 1, False) == 4 and fp.rows_per_wave(465, 465, 1, True) == 4
    assert fp.rows_per_wave(9, 2, 1, True, 7) == 6 and fp.rows_per_wave(9, 2, 1, True, 1) == 4
    assert all(fp.rows_per_wave(c["w"], c["h"], 1, True, c["rows"]) % 2 == 0 for c in GEOMETRY)


# ---- the kill matrix --------------------------------------------------------------------------------------------------
def can_occur(slip, case):
    """Whether a structure slip can change a byte at this shape at all (worked out from the kernel, not from the model's
    output): the bytes it would change exist and are stored."""
    h, w, (l, r, t, b) = case["h"], case["w"], case["crop"]
    cols, rows = range(l, w - r), range(t, h - b)
    rpw = fp.rows_per_wave(w, h, case["frames"], case["combined"], case["rows"])
    if not cols or not rows:
        return False
    return {
        "mid_max": w >= 2,                                          # (one column: the three mids of a window are one value)
        "left_own": w >= 2 and any(x % 4 == 0 for x in cols),       # column x - 1 against the lane's own column x + 3
        "right_own": any(x % 4 == 3 for x in cols),                 # column x + 1 against the lane's own column x - 3
        # x - 3 for x - 1 (both 0 in lane 1 of strip 0); one row and x the last column: the window is 3 x (a, b, b), median b
        "left_field_swapped": any(x % 4 == 0 and x >= 4 and (x < w - 1 or h >= 2) for x in cols),
        "right_field_swapped": any(x % 4 == 3 and x + 1 < w - 1 for x in cols),   # x + 3 for x + 1 (both w - 1 at the edge)
        "border_zero": 0 in rows or h - 1 in rows or 0 in cols or w - 1 in cols,  # a stored pixel on the image's border
        "border_reflect": (h >= 2 and (0 in rows or h - 1 in rows)) or (w >= 2 and (0 in cols or w - 1 in cols)),
        "seam_not_stored": any(x % fp.STRIP >= fp.STRIP - 4 for x in cols) or (case["combined"] and w > fp.STRIP - 4),
        # lane 0 of a later strip computes column x0 - 4 with column x0 - 1 for x0 - 5; lane 63 (if its first column is in
        # the image) computes column x0 + 251 with x0 + 248 for x0 + 252
        "halo_stores": any((x % fp.STRIP == fp.STRIP - 4 and x + 4 < w) or (x >= fp.STRIP and x % fp.STRIP == 3) for x in cols),
        "row_k1_wrong_third": h >= 2 and any(y % 2 == 1 for y in rows),
        "odd_last_row_dropped": h % 2 == 1 and h - 1 in rows,
        # (one column wide and on the image's last row the window is 3 x (row y - 1, y, y): median row y whatever stands above)
        "chunk_first_row_replicated": any(y > 0 and y % rpw == 0 and (y < h - 1 or w >= 2) for y in rows),
        "crop_on_combined": case["combined"] and case["crop"] != (0, 0, 0, 0),
        "combined_from_halo_row": case["combined"],
        "narrow_no_clamp": w < 4,
    }[slip]


def _kills(rule, frames, geo, slip):
    return any(not fp.same(fp.fuse_model(rule, six, geo, slip), want) for six, want in frames)


def _table_kills(rule, slip, names=None):
    out = {}
    for name, six, want in _table(rule):
        if names is None or name in names:
            geo = dict(crop=(0, 0, 0, 0), combined=True, rows=fp.rows_per_wave(six[0].shape[1], six[0].shape[0], 1, True))
            out[name] = not fp.same(fp.fuse_model(rule, six, geo, slip), fp.expected_as_model(*want))
    return out


RULE_SLIP_EDGE_CASES = tuple(k for k, c in enumerate(GEOMETRY) if (c["name"], c["h"], c["w"]) in (("size", 7, 497), ("seams", 31, 500))
                             or c["crop"] == gpu.REFERENCE_CROP)


@functools.lru_cache(maxsize=None)
def kill_matrix():
    """slip -> (rule_table, lively, median_edges) marks.  X: killed wherever it can occur; a number: on that many cases; a
    dot: nowhere."""
    rows, problems = {}, []
    for slip in fp.RULE_SLIPS:  # per rule it can be made in: its table (both kernels), every lively case, three edge cases
        rules = fp.SLIPS[slip]
        tab = [_table_kills(rule, slip, ("edges", "edges_narrow")) for rule in rules]
        assert all(t["edges"] and t["edges_narrow"] for t in tab), (slip, tab)  # each rule's wide and NARROW kernel
        live = sum(_kills(rule, *_frames(rule, k, "lively"), slip) for rule in rules for k in range(len(GEOMETRY)))
        edge = sum(_kills(rule, *_frames(rule, k, "edges"), slip) for rule in rules if rule in fp.PASS_THROUGH
                   for k in RULE_SLIP_EDGE_CASES)
        rows[slip] = ("X", str(live) if live else ".", str(edge) if edge else ".")
    for slip in fp.STRUCTURE_SLIPS:  # the structure is every rule's: one rule per case, in turn
        tab = _table_kills(fp.GRAD_FILTER, slip)
        marks = []
        per_case = np.zeros((len(GEOMETRY), 2), dtype=bool)
        for col, which in enumerate(("lively", "edges")):
            for k, case in enumerate(GEOMETRY):
                if which == "edges" and not case["edges"]:
                    continue
                rule = fp.RULES[k % 9] if which == "lively" else _edge_rule(k)
                per_case[k, col] = _kills(rule, *_frames(rule, k, which), slip)
        can = np.array([can_occur(slip, case) for case in GEOMETRY])
        short = lambda ks: [(k, GEOMETRY[k]["h"], GEOMETRY[k]["w"], GEOMETRY[k]["crop"], GEOMETRY[k]["rows"]) for k in ks[:8]]  # noqa: E731
        if per_case[~can].any():
            problems.append((slip, "killed where it cannot occur", short(np.flatnonzero(per_case.any(1) & ~can))))
        if (can & ~per_case.any(1)).any():
            problems.append((slip, "open on shapes where it can occur", short(np.flatnonzero(can & ~per_case.any(1)))))
        for col in range(2):
            n = int(per_case[:, col].sum())
            ran = np.array([c["edges"] or col == 0 for c in GEOMETRY])
            marks.append("X" if n and per_case[can & ran, col].all() else str(n) if n else ".")
        n_tab = sum(tab.values())
        rows[slip] = ("X" if n_tab == len(tab) else str(n_tab) if n_tab else ".", marks[0], marks[1])
    assert not problems, "\n".join(map(str, problems))
    return rows


def format_matrix(rows):
    lines = ["%-28s%-12s%-12s%s" % ("slip", "rule_table", "lively", "median_edges")]
    lines += ["%-28s%-12s%-12s%s" % ((slip,) + marks) for slip, marks in rows.items()]
    return "\n".join(lines)


KILL_MATRIX = """
slip                        rule_table  lively      median_edges
s1_thr                      X           228         .
s2_thr                      X           305         3
s2_thr_minus                X           438         .
s1_thr125                   X           .           .
s2_thr125                   X           .           .
d1_thr                      X           63          .
d2_thr                      X           58          .
tie_cam1                    X           284         .
tie_cam2                    X           210         .
avg_up                      X           326         .
half_dword                  X           302         .
sign_bit7                   X           805         6
ratio_lo_strict             X           56          .
ratio_hi_loose              X           .           .
shl2_8bit                   X           .           .
black_d1_only               X           119         .
mid_max                     4           116         X
left_own                    4           113         X
right_own                   4           98          X
left_field_swapped          4           92          X
right_field_swapped         4           87          X
border_zero                 X           117         X
border_reflect              .           117         X
seam_not_stored             4           X           X
halo_stores                 4           59          60
row_k1_wrong_third          X           102         X
odd_last_row_dropped        .           X           X
chunk_first_row_replicated  4           52          X
crop_on_combined            .           X           X
combined_from_halo_row      X           X           X
narrow_no_clamp             1           X           X
"""


def test_kill_matrix():
    """The matrix of tests/README.md.  Inside kill_matrix(): no structure slip is killed on a shape where it cannot
    occur, each is killed by lively or median_edges on every shape where it can, and each rule slip is killed by its
    rule's table in the wide and in the NARROW kernel's image."""
    text = format_matrix(kill_matrix())
    print(text)
    assert text.strip() == KILL_MATRIX.strip()
    assert set(kill_matrix()) == set(fp.SLIPS)
    for slip, marks in kill_matrix().items():
        assert marks[0] == "X" or marks[1] != "." or marks[2] != ".", (slip, "open")


# ---- the gap this closes ----------------------------------------------------------------------------------------------
def test_the_earlier_suite_never_gave_four_rules_their_own_s2_threshold():
    """test_fusion_gpu.py's inputs through the restated rule: its table takes s1 from `scores` and s2 from scores[::2] and
    compares the cell centres at eight d2 columns, plus one whole image at s1 = s2 = 110; its "uniform" / "thresholds"
    planes, the sessions and the address tests run GRAD_FILTER and BETTER_SCORE only.  With the constant s2 is compared
    with one too high, ONLY_GOOD_1 (s2 < 51), ONLY_GOOD_AVG (s2 < 101) and WEIGHTED_AVERAGE (s2 < 2) give the same bytes on
    all of that, and so does OVERLAP with the constant one too low (s2 < 19: s2 = 19 never occurs; s2 = 20 does, so its
    constant one too HIGH did show).  Each rule's table here shows the slip, in both kernels."""
    scores = np.array([0, 1, 2, 19, 20, 21, 49, 50, 99, 100, 101, 124, 125, 126, 229, 230, 255])
    assert set(scores[::2]) == {0, 2, 20, 49, 99, 101, 125, 229, 255}
    d1, d2 = np.meshgrid(np.arange(256), np.array([0, 1, 4, 5, 100, 229, 230, 255]), indexing="ij")
    d = np.arange(256, dtype=np.uint8)
    t1, t2 = (np.repeat(np.repeat(a, 3, axis=0), 3, axis=1) for a in np.meshgrid(d, d, indexing="ij"))
    # the s2 the slip needs: the constant itself for "+ 1" (s2 < t + 1 differs from s2 < t at s2 = t), t - 1 for "- 1"
    unseen = {fp.ONLY_GOOD_1: ("s2_thr", 50), fp.ONLY_GOOD_AVG: ("s2_thr", 100), fp.WEIGHTED_AVERAGE: ("s2_thr", 1),
              fp.OVERLAP: ("s2_thr_minus", 19)}
    for rule, (slip, needs) in unseen.items():
        other = "s2_thr_minus" if slip == "s2_thr" else "s2_thr"
        assert rule in fp.SLIPS[slip] and needs not in scores[::2] and needs in fp.score_edges(rule)
        seen_other = False
        for s1 in scores:
            for s2 in scores[::2]:  # a cell's centre is the rule's value: nine equal bytes
                a = fp.rule_fields(rule, d1, d2, s1, s2, d1 + d2, False)
                assert np.array_equal(a, fp.rule_fields(rule, d1, d2, s1, s2, d1 + d2, False, slip)), (rule, s1, s2)
                assert np.array_equal(a, fp.rules_ref(rule, d1, d2, s1, s2))
                seen_other |= not np.array_equal(a, fp.rule_fields(rule, d1, d2, s1, s2, d1 + d2, False, other))
        assert seen_other  # the constant off by one the other way did show there (OVERLAP: s2 = 20 is among scores[::2])
        six = [t1, t2, np.full_like(t1, 110), np.full_like(t1, 110), t1, t2]
        geo = dict(crop=(0, 0, 0, 0), combined=False, rows=fp.rows_per_wave(768, 768, 1, False))
        assert fp.same(fp.fuse_model(rule, six, geo, slip), fp.fuse_model(rule, six, geo))
        assert len(np.unique(fp.fuse_model(rule, six, geo)[0])) == 1  # ... and that image is constant under these rules
        kills = _table_kills(rule, slip, ("edges", "edges_narrow"))
        assert kills == {"edges": True, "edges_narrow": True}
    # under the default rule the planes do meet their thresholds: GRAD_FILTER's own s2 slip shows on "thresholds"
    rng = np.random.default_rng(465 * 7919 + 465 + len("thresholds"))
    edge = np.array([0, 1, 19, 20, 49, 50, 99, 100, 101, 124, 125, 126, 255], dtype=np.uint8)
    p1 = rng.integers(0, 256, size=(465, 465)).astype(np.uint8)
    p2 = np.clip(p1.astype(np.int32) + rng.integers(-40, 41, size=(465, 465)), 0, 255).astype(np.uint8)
    six = [p1, p2, rng.choice(edge, size=(465, 465)), rng.choice(edge, size=(465, 465)), p1, p2]
    geo = dict(crop=(0, 0, 0, 0), combined=False, rows=4)
    assert not fp.same(fp.fuse_model(fp.GRAD_FILTER, six, geo, "s2_thr"), fp.fuse_model(fp.GRAD_FILTER, six, geo))
