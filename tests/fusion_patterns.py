"""Built inputs for the depth-map fusion kernels (k_fuse_median3<RULE, NARROW> of d2pc_fusion.hip, the rule arithmetic
of d2pc_fuse_pair.hpp, k_node_fuse<16|64> of d2pc_node.hip), numpy only.

The expected answer of every test is oracle.fuse.  This module holds
  * rules_ref / median3 / fuse_ref: the nine rules (reference src/depth_map_fusion.cpp:162-235) and the 3 x 3 replicate
    median restated in plain integer numpy -- a second opinion on the oracle;
  * rule_table, lively, median_edges: the generators (tests/README.md, "Fusion patterns");
  * fuse_model: the STRUCTURE of the kernel restated (16-bit fields and sign masks, sorted vertical triples, neighbour
    columns from the neighbour lanes, halo lanes, 248-column strips, two rows per step, replicated borders, the crop, the
    combined plane) with one slip at a time.  It is never the expected answer; it says which mistakes the inputs show.
"""
import numpy as np

(WEIGHTED_AVERAGE, MAX_DIST, MAX_DIST_UNLESS_BLACK, BETTER_SCORE, ONLY_GOOD_1, ONLY_GOOD_AVG, OVERLAP, BLACK_TO_WHITE,
 GRAD_FILTER) = RULES = tuple(range(9))
RULE_NAMES = ("WEIGHTED_AVERAGE", "MAX_DIST", "MAX_DIST_UNLESS_BLACK", "BETTER_SCORE", "ONLY_GOOD_1", "ONLY_GOOD_AVG",
              "OVERLAP", "BLACK_TO_WHITE", "GRAD_FILTER")
STRIP = 248          # output columns of a wave: 62 lanes x 4 pixels
SENTINEL = 0xA5      # what the GPU file fills its buffers with; the model's out-of-plane reads see it too

# the score thresholds a rule compares against, and further scores its table holds (adjacent values for s1 < s2)
THRESHOLDS = {WEIGHTED_AVERAGE: (1,), MAX_DIST: (), MAX_DIST_UNLESS_BLACK: (), BETTER_SCORE: (), ONLY_GOOD_1: (50,),
              ONLY_GOOD_AVG: (100,), OVERLAP: (20,), BLACK_TO_WHITE: (), GRAD_FILTER: (100, 125)}
EXTRA_SCORES = {BETTER_SCORE: (1, 127, 128, 129), OVERLAP: (127, 128), BLACK_TO_WHITE: (1, 127, 128, 254)}
CLASSES = {WEIGHTED_AVERAGE: ("avg", "d1", "d2", "zero"), MAX_DIST: ("d1<d2", "d1>d2", "equal"),
           MAX_DIST_UNLESS_BLACK: ("black", "not_black"), BETTER_SCORE: ("d1", "d2"), ONLY_GOOD_1: ("d2", "zero"),
           ONLY_GOOD_AVG: ("avg", "zero"), OVERLAP: ("150", "255", "zero"), BLACK_TO_WHITE: ("255-s1",),
           GRAD_FILTER: ("d1", "d2", "avg", "zero")}
# one score pair of each outcome class whose output depends on the distances: the 65,536-pair tables
FULL_TABLE_SCORES = {WEIGHTED_AVERAGE: ((0, 0), (0, 5), (5, 0)), MAX_DIST: ((0, 0),), MAX_DIST_UNLESS_BLACK: ((0, 0),),
                     BETTER_SCORE: ((10, 20), (20, 10)), ONLY_GOOD_1: ((0, 49),), ONLY_GOOD_AVG: ((99, 99),), OVERLAP: (),
                     BLACK_TO_WHITE: ("scores",), GRAD_FILTER: ((10, 20), (20, 10), (110, 110))}
# edge distances: the ends (0..2: d < 1 from both sides), 229..231 (d < 230), 127..129 (|a - b| >= 128 against both ends), and pairs on and next to
# d1 / d2 = 4/5 (4 : 5, 160 : 200) and 5/4 (5 : 4, 250 : 200)
D_EDGE = (0, 1, 2, 3, 4, 5, 6, 127, 128, 129, 159, 160, 161, 199, 200, 201, 229, 230, 231, 249, 250, 251, 254, 255)


def _i64(*arrays):
    return [np.asarray(a).astype(np.int64) for a in np.broadcast_arrays(*arrays)]


# ---- the second opinion ---------------------------------------------------------------------------------------------
def ratio_ok(d1, d2):
    """gradFilter's 0.8 < float(d1) / float(d2) < 1.25 as tests/golden/make_fusion_golden.py has it: the quotient is a
    float32, the bounds are the double literals; d2 = 0 gives inf or NaN, which fail."""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (np.asarray(d1).astype(np.float32) / np.asarray(d2).astype(np.float32)).astype(np.float64)
        return (q > 0.8) & (q < 1.25)


def outcome_class(rule, d1, d2, s1, s2):
    """Index into CLASSES[rule] per pixel."""
    d1, d2, s1, s2 = _i64(d1, d2, s1, s2)
    if rule == WEIGHTED_AVERAGE:  # integer weights: 1 for a score of 0, else 0
        return np.select([(s1 == 0) & (s2 == 0), s1 == 0, s2 == 0], [0, 1, 2], 3)
    if rule == MAX_DIST:
        return np.select([d1 < d2, d1 > d2], [0, 1], 2)
    if rule == MAX_DIST_UNLESS_BLACK:
        return np.where((d1 == 0) | (d2 == 0), 0, 1)
    if rule == BETTER_SCORE:
        return np.where(s1 < s2, 0, 1)
    if rule == ONLY_GOOD_1:
        return np.where(s2 < 50, 0, 1)
    if rule == ONLY_GOOD_AVG:
        return np.where((s1 < 100) & (s2 < 100), 0, 1)
    if rule == OVERLAP:
        return np.select([(s1 < s2) & (s1 < 20), (s2 < s1) & (s2 < 20)], [0, 1], 2)
    if rule == BLACK_TO_WHITE:
        return np.zeros(np.broadcast(d1, d2, s1, s2).shape, dtype=np.int64)
    assert rule == GRAD_FILTER
    cam1 = (s1 < s2) & (s1 < 100) & (d1 < 230)
    cam2 = (s2 < s1) & (s2 < 100) & (d2 < 230)
    both = ratio_ok(d1, d2) & (s1 < 125) & (s2 < 125)  # score < 1.25 * 100
    return np.select([cam1, cam2, both], [0, 1, 2], 3)


def rules_ref(rule, d1, d2, s1, s2):
    """The fused byte per pixel, before the median."""
    cls = outcome_class(rule, d1, d2, s1, s2)
    d1, d2, s1, s2 = _i64(d1, d2, s1, s2)
    zero, avg = np.zeros_like(cls), (d1 + d2) // 2
    values = {WEIGHTED_AVERAGE: (avg, d1, d2, zero), MAX_DIST: (d1, d2, d1),
              MAX_DIST_UNLESS_BLACK: (np.maximum(d1, d2), np.minimum(d1, d2)), BETTER_SCORE: (d1, d2),
              ONLY_GOOD_1: (d2, zero), ONLY_GOOD_AVG: (avg, zero), OVERLAP: (zero + 150, zero + 255, zero),
              BLACK_TO_WHITE: (255 - s1,), GRAD_FILTER: (d1, d2, avg, zero)}[rule]
    out = np.select([cls == k for k in range(len(values))], [np.broadcast_to(v, cls.shape) for v in values])
    return out.astype(np.uint8)


def median3(img):
    """3 x 3 median with replicated borders, from nine shifted views."""
    h, w = img.shape
    p = np.pad(img, 1, mode="edge")
    views = np.stack([p[i:i + h, j:j + w] for i in range(3) for j in range(3)])
    return np.sort(views, axis=0)[4]


def fuse_ref(rule, planes, crop=(0, 0, 0, 0), want_combined=True):
    """oracle.fuse's answer by rules_ref and median3."""
    l, r, t, b = crop
    h, w = planes[0].shape
    med = median3(rules_ref(rule, *planes[:4]))
    comb = np.minimum(planes[4], planes[5]) if want_combined else None
    return med[t:h - b, l:w - r], comb


# ---- generators -----------------------------------------------------------------------------------------------------
def score_edges(rule):
    s = {0, 255} | set(EXTRA_SCORES.get(rule, ()))
    for t in THRESHOLDS[rule]:
        s |= {t - 1, t, t + 1}
    return tuple(sorted(s))


def _cells(a):
    return np.ascontiguousarray(np.repeat(np.repeat(a, 3, axis=0), 3, axis=1).astype(np.uint8))


def rule_table(rule):
    """-> [(name, [d1, d2, s1, s2])]: images of 3 x 3 cells constant in all four inputs (3 wide against 4 pixels per
    lane: every byte lane and both 16-bit fields meet every cell).  "edges": S x S score pairs (rows: s1, columns: s2)
    of D x D distances (rows: d1, columns: d2); then one image of all 65,536 (d1, d2) pairs per entry of
    FULL_TABLE_SCORES (BLACK_TO_WHITE: all (s1, s2) pairs instead).  The cell values are planes[:, 1::3, 1::3]."""
    S, D = np.array(score_edges(rule)), np.array(D_EDGE)
    outer, inner = np.repeat(np.arange(len(S)), len(D)), np.tile(np.arange(len(D)), len(S))
    s1, s2 = np.meshgrid(S[outer], S[outer], indexing="ij")
    d1, d2 = np.meshgrid(D[inner], D[inner], indexing="ij")
    out = [("edges", [_cells(d1), _cells(d2), _cells(s1), _cells(s2)])]
    a, b = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    for pair in FULL_TABLE_SCORES[rule]:
        if pair == "scores":
            out.append(("all_scores", [_cells(b), _cells(a), _cells(a), _cells(b)]))
        else:
            out.append(("all_distances_%d_%d" % pair, [_cells(a), _cells(b), _cells(np.full_like(a, pair[0])),
                                                       _cells(np.full_like(a, pair[1]))]))
    for _, planes in out:
        assert max(planes[0].shape) <= 768
    # the S x S x D x D cells once more, one below the other in an image three pixels wide: the NARROW kernels are
    # compiled separately and would otherwise meet their rule's thresholds by chance only
    tall = lambda a: np.ascontiguousarray(np.repeat(np.repeat(a[1::3, 1::3].reshape(-1), 3)[:, None], 3, axis=1))  # noqa: E731
    out.insert(1, ("edges_narrow", [tall(p) for p in out[0][1]]))
    return out


def lively(rule, rng, h, w):
    """-> [d1, d2, s1, s2], (h, w) bytes: the outcome class is drawn per pixel first (balanced: a permutation of the
    pixels modulo the number of classes), then scores and distances that realise it."""
    n, ncls = h * w, len(CLASSES[rule])
    cls = (rng.permutation(n) % ncls).reshape(h, w)
    U = lambda lo, hi: rng.integers(lo, np.asarray(hi) + 1, size=(h, w))  # noqa: E731  inclusive, hi may be an array
    coin = rng.integers(0, 2, size=(h, w)).astype(bool)
    d1, d2, s1, s2 = U(0, 255), U(0, 255), U(0, 255), U(0, 255)
    pick = lambda options: np.select([cls == k for k in range(ncls)], options)  # noqa: E731
    if rule == WEIGHTED_AVERAGE:
        nz1, nz2 = U(1, 255), U(1, 255)
        s1, s2 = pick([0 * nz1, 0 * nz1, nz1, nz1]), pick([0 * nz2, nz2, 0 * nz2, nz2])
    elif rule == MAX_DIST:
        lo = U(0, 254)
        hi = U(lo + 1, 255)
        d1, d2 = pick([lo, hi, d1]), pick([hi, lo, d1])
    elif rule == MAX_DIST_UNLESS_BLACK:
        p1, p2 = U(1, 255), U(1, 255)
        both = rng.integers(0, 8, size=(h, w)) == 0
        d1, d2 = pick([np.where(coin | both, 0, p1), p1]), pick([np.where(~coin | both, 0, p2), p2])
    elif rule == BETTER_SCORE:
        lo = U(0, 254)
        hi = U(lo + 1, 255)
        ge = U(s2, 255)
        s1, s2 = pick([lo, ge]), pick([hi, s2])
    elif rule == ONLY_GOOD_1:
        s2 = pick([U(0, 49), U(50, 255)])
    elif rule == ONLY_GOOD_AVG:
        g1, g2, b1, b2 = U(0, 99), U(0, 99), U(100, 255), U(100, 255)
        both = rng.integers(0, 4, size=(h, w)) == 0
        s1, s2 = pick([g1, np.where(coin | both, b1, g1)]), pick([g2, np.where(~coin | both, b2, g2)])
    elif rule == OVERLAP:
        lo = U(0, 19)
        hi = U(lo + 1, 255)
        z = U(20, 255)
        s1, s2 = pick([lo, hi, np.where(coin, z, lo)]), pick([hi, lo, np.where(coin, U(20, 255), lo)])
    elif rule == GRAD_FILTER:
        lo = U(0, 99)
        hi = U(lo + 1, 255)
        near = U(229 - 40, 229)  # camera's own depth below 230, often close to it
        eq, m1, m2 = U(0, 124), U(100, 124), U(100, 124)
        b2_ = U(5, 255)
        b1_ = U((4 * b2_ + 4) // 5, np.minimum(255, (5 * b2_ - 1) // 4))
        s1 = pick([lo, hi, np.where(coin, eq, m1), U(125, 255)])
        s2 = pick([hi, lo, np.where(coin, eq, m2), U(125, 255)])
        d1 = pick([np.where(coin, near, U(0, 229)), d1, b1_, d1])
        d2 = pick([d2, np.where(coin, near, U(0, 229)), b2_, d2])
    planes = [p.astype(np.uint8) for p in (d1, d2, s1, s2)]
    assert np.array_equal(outcome_class(rule, *planes), cls), RULE_NAMES[rule]
    return planes


PASS_THROUGH = tuple(r for r in RULES if r != OVERLAP)  # the rules that can hand a plane to the median unchanged


def pass_through(rule, plane):
    """[d1, d2, s1, s2] under which `rule` fuses to `plane` everywhere (bytes 1..229): one camera wins at every pixel;
    for MAX_DIST the other distance is 255; BLACK_TO_WHITE passes 255 - s1."""
    assert rule in PASS_THROUGH and plane.min() >= 1 and plane.max() <= 229
    c = lambda v: np.full_like(plane, v)  # noqa: E731
    return {WEIGHTED_AVERAGE: [plane, c(50), c(0), c(1)], MAX_DIST: [plane, c(255), c(3), c(4)],
            MAX_DIST_UNLESS_BLACK: [plane, c(255), c(3), c(4)], BETTER_SCORE: [plane, c(50), c(0), c(1)],
            ONLY_GOOD_1: [c(50), plane, c(9), c(0)], ONLY_GOOD_AVG: [plane, plane, c(0), c(0)],
            BLACK_TO_WHITE: [c(50), c(60), 255 - plane, c(4)], GRAD_FILTER: [plane, c(50), c(10), c(90)]}[rule]


FIXED = 13  # edge_frames: the stripes, the checkerboard and the noise come first


def _place(items, h, w, bg):
    """Greedy: every item (y, x, 3 x 3 patch) into the first frame in which no earlier item's centre lies within two
    pixels in y and in x, so that patches never overlap and a single pixel stays alone in every window that holds it."""
    frames, centres = [], []
    for y, x, patch in items:
        for f in range(len(frames) + 1):
            if f == len(frames):
                frames.append(np.full((h, w), bg, dtype=np.uint8))
                centres.append([])
            if all(max(abs(y - yy), abs(x - xx)) >= 3 for yy, xx in centres[f]):
                break
        for dy in range(3):
            for dx in range(3):
                yy, xx = y + dy - 1, x + dx - 1
                if 0 <= yy < h and 0 <= xx < w and patch[dy][dx] is not None:
                    frames[f][yy, xx] = patch[dy][dx]
        centres[f].append((y, x))
    return frames


def edge_frames(h, w, seams_x=(247, 248, 495, 496), seams_y=(3, 4, 7, 8, 15, 16), lo=7, hi=201):
    """-> (F, h, w) two-level planes: stripes of period 2, 3, 4 in x and in y, a checkerboard and six frames of seeded
    two-level noise (FIXED = 13 frames); 3 x 3 blocks of
    exactly c = 0..9 high pixels centred on every seam column; a single bright pixel on a dark plane and a single dark
    one on a bright plane at every x mod 4 beside column 0, column w - 1 and the seams, in the first and last rows, a
    chunk's first and last rows (seams_y) and so the corners.  Returns the frames and where the count blocks lie:
    {(seam column, c): (frame, row)}."""
    yy, xx = np.mgrid[0:h, 0:w]
    two = lambda mask: np.where(mask, hi, lo).astype(np.uint8)  # noqa: E731
    frames = [two(xx % p == 0) for p in (2, 3, 4)] + [two(yy % p == 0) for p in (2, 3, 4)] + [two((xx + yy) % 2 == 0)]
    rng = np.random.default_rng(1000 * h + w)  # ... and two-level noise, three densities twice: windows of every count anywhere
    frames += [two(rng.random((h, w)) < dens) for dens in (0.3, 0.5, 0.7, 0.3, 0.5, 0.7)]
    cols = sorted({x for x in list(range(0, 4)) + list(range(w - 4, w)) + [x + d for x in seams_x for d in range(-3, 5)]
                   if 0 <= x < w})
    rows = sorted({y for y in (0, 1, h - 2, h - 1) + tuple(seams_y) if 0 <= y < h})
    none = [[None] * 3 for _ in range(3)]
    single = lambda v: [none[0], [None, v, None], none[2]]  # noqa: E731
    blocks, block_rows = [], list(range(1, h - 1, 3))
    for x in seams_x:
        if 1 <= x <= w - 2 and block_rows:
            for c in range(10):
                patch = [[hi if 3 * dy + dx < c else lo for dx in range(3)] for dy in range(3)]
                blocks.append((block_rows[c % len(block_rows)], x, patch, c))
    dark = _place([(b[0], b[1], b[2]) for b in blocks], h, w, lo) + _place([(y, x, single(hi)) for y in rows for x in cols], h, w, lo)
    where = {}
    for y, x, patch, c in blocks:  # find each block again (the greedy placement is deterministic)
        want = np.array(patch, dtype=np.uint8)
        where[(x, c)] = next((len(frames) + f, y) for f, fr in enumerate(dark)
                             if np.array_equal(fr[y - 1:y + 2, x - 1:x + 2], want))
    bright = _place([(y, x, single(lo)) for y in rows for x in cols], h, w, hi)
    return np.stack(frames + dark + bright), where


def median_edges(rule, h, w, **kw):
    """-> [d1, d2, s1, s2] of shape (F, h, w) that fuse to edge_frames(h, w) under a pass-through rule."""
    return pass_through(rule, edge_frames(h, w, **kw)[0])


# ---- the kernel's structure, with one slip at a time ------------------------------------------------------------------
def rows_per_wave(w, h, frames, combined, hint=0):
    """launch_fuse's choice of the rows a wave walks (always even)."""
    if 2 <= hint <= 1024:
        return hint & ~1
    strips, rows = -(-w // STRIP), 8 if combined else 16
    while rows > 4 and strips * -(-h // rows) * frames < 2048:
        rows >>= 1
    return rows


# slip -> the rules whose code it can be made in (None: the structure, which all rules share)
SLIPS = {
    "s1_thr": (WEIGHTED_AVERAGE, ONLY_GOOD_AVG, OVERLAP, GRAD_FILTER),   # the constant s1 is compared with, + 1
    "s2_thr": (WEIGHTED_AVERAGE, ONLY_GOOD_1, ONLY_GOOD_AVG, OVERLAP, GRAD_FILTER),
    "s2_thr_minus": (WEIGHTED_AVERAGE, ONLY_GOOD_1, ONLY_GOOD_AVG, OVERLAP, GRAD_FILTER),   # ... - 1
    "s1_thr125": (GRAD_FILTER,), "s2_thr125": (GRAD_FILTER,),
    "d1_thr": (MAX_DIST_UNLESS_BLACK, GRAD_FILTER), "d2_thr": (MAX_DIST_UNLESS_BLACK, GRAD_FILTER),
    "tie_cam1": (BETTER_SCORE, OVERLAP, GRAD_FILTER),                   # s1 < s2 as s1 <= s2
    "tie_cam2": (OVERLAP, GRAD_FILTER),                                 # s2 < s1 as s2 <= s1
    "avg_up": (WEIGHTED_AVERAGE, ONLY_GOOD_AVG, GRAD_FILTER),
    "half_dword": (WEIGHTED_AVERAGE, ONLY_GOOD_AVG, GRAD_FILTER),       # >> 1 on the dword: a field leaks into its neighbour
    "sign_bit7": (WEIGHTED_AVERAGE, MAX_DIST_UNLESS_BLACK, BETTER_SCORE, ONLY_GOOD_1, ONLY_GOOD_AVG, OVERLAP, GRAD_FILTER),
    "ratio_lo_strict": (GRAD_FILTER,), "ratio_hi_loose": (GRAD_FILTER,), "shl2_8bit": (GRAD_FILTER,),
    "black_d1_only": (MAX_DIST_UNLESS_BLACK,),
    "mid_max": None, "left_own": None, "right_own": None, "left_field_swapped": None, "right_field_swapped": None,
    "border_zero": None, "border_reflect": None, "seam_not_stored": None, "halo_stores": None,
    "row_k1_wrong_third": None, "odd_last_row_dropped": None, "chunk_first_row_replicated": None,
    "crop_on_combined": None, "combined_from_halo_row": None, "narrow_no_clamp": None,
}
RULE_SLIPS = tuple(s for s, r in SLIPS.items() if r is not None)
STRUCTURE_SLIPS = tuple(s for s, r in SLIPS.items() if r is None)


def rule_fields(rule, d1, d2, s1, s2, partner_sum, low_field, slip=None):
    """fuse_pair per pixel: the value of the pixel's 16-bit field.  a < b is the sign bit of the field a - b; the signs
    of one condition are AND-ed as bits; the result is picked with masks.  partner_sum is d1 + d2 of the pixel two
    columns on, which shares the dword (low_field: this pixel is the low one of the two)."""
    d1, d2, s1, s2, partner_sum = _i64(d1, d2, s1, s2, partner_sum)
    sub = lambda a, b: (a - b) & 0xFFFF  # noqa: E731
    sign = lambda v: ((v >> (7 if slip == "sign_bit7" else 15)) & 1).astype(bool)  # noqa: E731
    bump = lambda name: 1 if slip == name else -1 if slip == name + "_minus" else 0  # noqa: E731
    avg = (d1 + d2 + bump("avg_up")) >> 1
    if slip == "half_dword":
        avg = avg | np.where(low_field, (partner_sum & 1) << 15, 0)
    s2_for_1, s1_for_2 = s2 + bump("tie_cam1"), s1 + bump("tie_cam2")
    if rule == WEIGHTED_AVERAGE:
        w1, w2 = sign(sub(s1, 1 + bump("s1_thr"))), sign(sub(s2, 1 + bump("s2_thr")))
        return np.where(w1, np.where(w2, avg, d1), np.where(w2, d2, 0))
    if rule == MAX_DIST:
        return np.minimum(d1, d2)
    if rule == MAX_DIST_UNLESS_BLACK:
        black = sign(sub(d1, 1 + bump("d1_thr")) | (0 if slip == "black_d1_only" else sub(d2, 1 + bump("d2_thr"))))
        return np.where(black, np.maximum(d1, d2), np.minimum(d1, d2))
    if rule == BETTER_SCORE:
        return np.where(sign(sub(s1, s2_for_1)), d1, d2)
    if rule == ONLY_GOOD_1:
        return np.where(sign(sub(s2, 50 + bump("s2_thr"))), d2, 0)
    if rule == ONLY_GOOD_AVG:
        return np.where(sign(sub(s1, 100 + bump("s1_thr")) & sub(s2, 100 + bump("s2_thr"))), avg, 0)
    if rule == OVERLAP:
        a = sign(sub(s1, s2_for_1) & sub(s1, 20 + bump("s1_thr")))
        b = sign(sub(s2, s1_for_2) & sub(s2, 20 + bump("s2_thr")))
        return np.where(a, 150, np.where(b, 255, 0))
    if rule == BLACK_TO_WHITE:
        return 255 - s1
    a = sign(sub(s1, s2_for_1) & sub(s1, 100 + bump("s1_thr")) & sub(d1, 230 + bump("d1_thr")))
    b = sign(sub(s2, s1_for_2) & sub(s2, 100 + bump("s2_thr")) & sub(d2, 230 + bump("d2_thr")))
    # 5 d1 >= 4 d2 and 4 d1 < 5 d2  <=>  t + d1 >= 0 and t - d2 < 0  with  t = 4 (d1 - d2)
    t = (sub(d1, d2) << 2) & 0xFFFF
    if slip == "shl2_8bit":
        t = t & 0xFF
        t = np.where(t >= 128, t - 256, t) & 0xFFFF
    lo_ok = sub(0, (t + d1) & 0xFFFF) if slip == "ratio_lo_strict" else ~((t + d1) & 0xFFFF) & 0xFFFF
    hi_ok = sub(t, d2 + bump("ratio_hi_loose"))
    c = sign(lo_ok & hi_ok & sub(s1, 125 + bump("s1_thr125")) & sub(s2, 125 + bump("s2_thr125")))
    return np.where(a, d1, np.where(b, d2, np.where(c, avg, 0)))


def fuse_model(rule, planes, geometry, slip=None):
    """One frame through the restated kernel.  planes: six (h, w) byte arrays; geometry: {"crop": (l, r, t, b), "rows":
    rows per wave, "combined": bool}.  -> (fused, combined) as int16, -1 where nothing was stored; the combined plane
    comes with one guard row above and two below (rows 1 .. h are the plane), None without "combined".

    Rows per wave are even, so the second output of a step (row k + 1) is an odd image row, only the image's last
    chunk can have an odd number of rows, and a chunk's first row is a multiple of "rows": the walk down a strip is
    restated over whole columns.  Out-of-plane bytes (NARROW without its clamp) read SENTINEL."""
    assert slip is None or slip in SLIPS
    d1, d2, s1, s2, g1, g2 = _i64(*planes)
    h, w = d1.shape
    l, r, t, b = geometry["crop"]
    cx0, cx1, cy0, cy1 = l, w - r, t, h - b
    rpw = geometry["rows"]
    cols = np.arange(w)
    fields = rule_fields(rule, d1, d2, s1, s2, (d1 + d2)[:, np.minimum(cols + 2, w - 1)], (cols % 4 < 2)[None, :], slip)
    # row h and column w: a zero border; column w + 1: what lies beside the plane
    F = np.zeros((h + 1, w + 2), dtype=np.int64)
    F[:h, :w] = fields
    F[:h, w + 1] = rule_fields(rule, *[np.int64(SENTINEL)] * 4, np.int64(2 * SENTINEL), False, slip)

    def at(i, n, is_col):  # load coordinate -> index into F
        i = np.asarray(i)
        if is_col and slip == "narrow_no_clamp" and w < 4:
            return np.where((i < 0) | (i >= n), n + 1, i)
        if slip == "border_zero":
            return np.where((i < 0) | (i >= n), n, i)
        if slip == "border_reflect":
            j = np.abs(i)
            return np.clip(np.where(j >= n, 2 * (n - 1) - j, j), 0, n - 1)
        return np.clip(i, 0, n - 1)

    # sorted vertical triples: rows y - 1, y, y + 1.  A step sorts the pair (k + 1, k + 2) once for both of its outputs:
    # row k + 1 adds row k, row k + 2 adds row k + 3 (slip: row k again, so an odd image row y sees y - 2, y - 1, y)
    y = np.arange(h)
    up = np.where(y % rpw == 0, y, y - 1) if slip == "chunk_first_row_replicated" else y - 1
    third = np.where(y % 2 == 1, y - 2, y + 1) if slip == "row_k1_wrong_third" else y + 1
    ra, rb, rc = F[at(up, h, False)], F[y], F[at(third, h, False)]
    lo = np.minimum(np.minimum(ra, rb), rc)
    hi = np.maximum(np.maximum(ra, rb), rc)
    me = ra + rb + rc - lo - hi
    med3 = lambda p, q, s: p + q + s - np.minimum(np.minimum(p, q), s) - np.maximum(np.maximum(p, q), s)  # noqa: E731

    oh, ow = max(cy1 - cy0, 0), max(cx1 - cx0, 0)
    fused = np.full((oh, ow), -1, dtype=np.int16)
    out_rows = np.arange(cy0, cy1)
    if slip == "odd_last_row_dropped" and h % 2 == 1:
        out_rows = out_rows[out_rows != h - 1]
    late = []  # what the halo lanes store lands after the owners' bytes
    slot = np.arange(min(256, 4 * (-(-w // 4) + 2)))  # (the lanes past the image's last are left out: they store nothing)
    lane, p = slot // 4, slot % 4
    for x0 in range(0, w, STRIP):
        xs = x0 - 4 + slot  # lane 0 = left halo, lane 63 = right halo
        left, right = slot - 1, slot + 1  # column -1 is the left lane's column 3, column 4 the right lane's column 0
        left[0], right[-1] = 3, len(slot) - 4     # the wave's end lanes get their own register back
        if slip == "left_own":
            left = np.where(p == 0, slot + 3, left)
        if slip == "right_own":
            right = np.where(p == 3, slot - 3, right)
        if slip == "left_field_swapped":   # the left lane's column 1 for its column 3
            left = np.where((p == 0) & (lane > 0), slot - 3, left)
        if slip == "right_field_swapped":  # the right lane's column 2 for its column 0
            right = np.where((p == 3) & (lane < 63), slot + 3, right)
        C, L, R = at(xs, w, True), at(x0 - 4 + left, w, True), at(x0 - 4 + right, w, True)
        mids = np.maximum(np.maximum(me[:, L], me[:, C]), me[:, R]) if slip == "mid_max" else med3(me[:, L], me[:, C], me[:, R])
        out = med3(np.maximum(np.maximum(lo[:, L], lo[:, C]), lo[:, R]), mids,
                   np.minimum(np.minimum(hi[:, L], hi[:, C]), hi[:, R]))
        # outE | (outO << 8): a field above 255 spills into the next pixel's byte
        byte = (out & 0xFF) | np.where(p >= 1, (np.roll(out, 1, axis=1) >> 8) & 0xFF, 0)
        lane_x = x0 - 4 + 4 * lane
        owner = (lane >= 1) & (lane <= (61 if slip == "seam_not_stored" else 62)) & (lane_x < w)
        for who, sink in ((owner, None), ((lane_x < w) & ((lane == 0) | (lane == 63)), late)):
            if sink is not None and slip != "halo_stores":
                continue
            keep = who & (xs >= cx0) & (xs < cx1)
            if sink is None:
                fused[np.ix_(out_rows - cy0, xs[keep] - cx0)] = byte[np.ix_(out_rows, keep)]
            else:
                sink.append((xs[keep] - cx0, byte[np.ix_(out_rows, keep)]))
    for where, what in late:
        fused[np.ix_(out_rows - cy0, where)] = what
    combined = None
    if geometry["combined"]:
        m = np.minimum(g1, g2)
        combined = np.full((h + 3, w), -1, dtype=np.int16)
        if slip == "crop_on_combined":
            combined[1:1 + oh, :ow] = m[cy0:cy1, cx0:cx1]
        else:
            combined[1:h + 1] = m
        if slip == "seam_not_stored":
            combined[:, (cols % STRIP) >= STRIP - 4] = -1
        if slip == "combined_from_halo_row":  # window rows 0 and rows + 1 (and rows + 2 below an odd chunk)
            combined[0], combined[h + 1] = m[0], m[h - 1]
            if h % 2 == 1:
                combined[h + 2] = m[h - 1]
    return fused, combined


def expected_as_model(fused, combined):
    """oracle.fuse's pair in the form fuse_model returns."""
    comb = None
    if combined is not None:
        comb = np.full((combined.shape[0] + 3, combined.shape[1]), -1, dtype=np.int16)
        comb[1:-2] = combined
    return fused.astype(np.int16), comb


def same(a, b):
    return np.array_equal(a[0], b[0]) and (a[1] is None) == (b[1] is None) and (a[1] is None or np.array_equal(a[1], b[1]))
