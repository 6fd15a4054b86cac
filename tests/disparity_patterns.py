"""Seeded disparity frames for the reprojection kernels (numpy only): the float-valued counterpart of value_patterns.py.

The suite's disparities come from uniform(0.5, 128) or k/8: seven binades out of 277, all positive, W never near zero,
no coordinate near overflow or underflow.  Each generator below says what it is built to reach;
tests/test_disparity_patterns.py checks that it does, from the exact reference alone (tests/exact_reproject.py), at the
shapes the GPU tests use (SHAPES).

Every generator returns a Pattern: `frames` (n, h, w) in its dtype, the Q and border it was built for, and the records
a test needs to find the interesting pixels again (`placed`: one row (frame, row, col, value index or group) per pixel
that was laid down on purpose).  The background of the float frames is the reference's own input, d = k/8, k in 1..255.
"""
import math
from fractions import Fraction
from types import SimpleNamespace

import numpy as np

from exact_reproject import OVERFLOW_THRESHOLD, f32_bits, make_q_default, round_fraction_to_f32

# name -> (width, height, border, row stride in elements of the host frame)
#   native : the reference's geometry; ROI start and width are multiples of four floats and the rows are 16-byte
#            aligned, so fp32 takes the 16-byte load path of tile_load_d
#   ragged : odd border, odd width, padded row stride: the scalar load path
#   border0: the whole frame is the ROI
# (the two small ROIs still hold 65,536 pixels, one per 16-bit raw value)
SHAPES = {"native": (752, 480, 40, 752), "ragged": (333, 221, 7, 341), "border0": (328, 208, 0, 328)}


def rig_q(w, h, **kw):
    """cv::stereoRectify's Q for the reference rig with its principal point at the centre of a w x h frame: as at
    752 x 480, u + cx is about 5e-4 in the column right of the centre (1e-3 at an odd width) and v + cy crosses zero
    in the middle of the frame."""
    args = dict(cx=(w + w % 2) / 2.0, cy=h / 2.0, nx=w, ny=h)
    args.update(kw)
    return make_q_default(**args)


def w_safe(q, width, height, border):
    """QStereo::w_safe as the host forms it (w_safe_for, d2pc_capi_route.hip), restated from its definition: 2^-126
    times a bound on the frame's largest |numerator| -- |f|, |u + cx| over the columns 0..width, |v + cy| over the
    rows 0..(last ROI row + 1).  |W| at least this large keeps every quotient below 2^126."""
    cx, cy, f = float(q[3]), float(q[7]), float(q[11])
    mx = max(abs(cx), abs(cx + width))
    my = max(abs(cy), abs(cy + (height - border)))
    return math.ldexp(max(abs(f), mx, my), -126)


def pitched(frame, pitch, fill=77):
    """`frame` as a view of a buffer whose rows are `pitch` elements apart; the pad columns hold `fill`."""
    h, w = frame.shape
    buf = np.full((h, pitch), fill, dtype=frame.dtype)
    buf[:, :w] = frame
    return buf[:, :w]


def _background(rng, n, h, w):
    return rng.integers(1, 256, size=(n, h, w)).astype(np.float32) / np.float32(8)


def _bits_to_f32(bits):
    return np.asarray(bits, dtype=np.uint32).view(np.float32)


def principal_cols(q, w, border):
    """The ROI columns either side of the principal point (u + cx changes sign between them)."""
    c0 = int(math.floor(-float(q[3])))
    return [c for c in (c0, c0 + 1) if border <= c < w - border]


def _rows_by_side(q, h, border):
    cy = float(q[7])
    rows = np.arange(border, h - border)
    return rows[rows + cy < 0], rows[rows + cy > 0]


def _place(rng, values, q, w, h, border, n_rand_cols):
    """Lay float32 `values` down in k/8 frames.  Every value sits once in each of the PROMISED columns -- the two
    columns either side of the principal point, the first and the last ROI column -- and in `n_rand_cols` seeded
    columns between them; in the two principal columns it sits on opposite sides of cy, in the others in seeded rows.
    One frame holds 2 * min(rows above cy, rows below cy) values; as many frames as it takes.
    -> (frames, placed (P, 4) int32 rows of (frame, row, col, value index), promised columns)."""
    above, below = _rows_by_side(q, h, border)
    m = min(len(above), len(below))
    cap = 2 * m
    promised = principal_cols(q, w, border) + [border, w - border - 1]
    assert len(set(promised)) == 4, promised
    n_frames = -(-len(values) // cap)
    frames = _background(rng, n_frames, h, w)
    placed = []
    all_rows = np.arange(border, h - border)
    for f in range(n_frames):
        chunk = np.arange(f * cap, min((f + 1) * cap, len(values)))
        free = np.setdiff1d(np.arange(border + 1, w - border - 1), promised)
        cols = promised + sorted(rng.choice(free, size=n_rand_cols, replace=False).tolist())
        a, b = rng.permutation(above)[:m], rng.permutation(below)[:m]
        side0, side1 = np.concatenate([a, b]), np.concatenate([b, a])
        for j, c in enumerate(cols):
            rows = side0 if j == 0 else side1 if j == 1 else rng.permutation(all_rows)[:cap]
            for i, vi in enumerate(chunk):
                frames[f, rows[i], c] = values[vi]
                placed.append((f, rows[i], c, vi))
    return frames, np.array(placed, dtype=np.int32), promised


# ---------------------------------------------------------------------------------------------------------------
def sweep_values(rng):
    """The values of binade_sweep as uint32 bit patterns: per exponent 2^-149 .. 2^127 the mantissas 1.0, 1 + ulp,
    2 - ulp and one seeded random (subnormal binades: the same four positions on their coarser grid, fewer where
    they coincide), both signs; then +-0, FLT_MIN, the largest subnormal, FLT_MAX and its lower neighbour, +-inf, NaN."""
    bits = []
    for e in range(-149, 128):
        if e >= -126:
            base = (e + 127) << 23
            row = [base, base | 1, base | 0x7FFFFF, base | int(rng.integers(2, 0x7FFFFF))]
        else:
            lo = 1 << (e + 149)
            hi = 2 * lo - 1
            row = [lo, min(lo + 1, hi), hi, int(rng.integers(lo, hi + 1))]
        for b in dict.fromkeys(row):
            bits += [b, b | 0x80000000]
    bits += [0, 0x80000000, 0x00800000, 0x007FFFFF, 0x7F7FFFFF, 0x7F7FFFFE, 0x7F800000, 0xFF800000, 0x7FC00000]
    return np.array(list(dict.fromkeys(bits)), dtype=np.uint32)


def f32_exponent(bits):
    """floor(log2 |x|) of finite non-zero float32 bit patterns, subnormals included."""
    mag = np.asarray(bits, dtype=np.uint32).astype(np.int64) & 0x7FFFFFFF
    field = mag >> 23
    sub = np.array([int(x).bit_length() - 150 for x in mag.reshape(-1)]).reshape(mag.shape)
    return np.where(field > 0, field - 127, sub)


def binade_sweep(seed, shape="native", n_rand_cols=2):
    """Every float32 binade from the smallest subnormal to 2^127, both signs, four mantissas each, and the specials
    (sweep_values), each value in the columns either side of the principal point, in the first and last ROI column
    and in seeded columns between, on both sides of cy (_place).

    Built to reach: Z = f / (a d) overflows for |d| below about 2^-122 and is subnormal-free but X = (u + cx) / (a d)
    in the principal columns (|u + cx| ~ 5e-4) falls into the float32 subnormal range for |d| above about 2^112 --
    a kernel that flushes subnormal results, or subnormal inputs (d below 2^-126: Z is +-inf either way, but X and Y
    must keep their signs), or loses the sign of a zero or an infinity, differs here; d == FLT_MAX takes the Z = 10000
    rule and its neighbour does not; +-0, +-inf and NaN have no exact answer and are compared with the oracle."""
    w, h, border, _ = SHAPES[shape]
    rng = np.random.default_rng((seed, 1, w, h))
    q = rig_q(w, h)
    values = sweep_values(rng)
    frames, placed, promised = _place(rng, _bits_to_f32(values), q, w, h, border, n_rand_cols)
    return SimpleNamespace(name="binade_sweep", shape=shape, q=q, border=border, frames=frames, placed=placed,
                           values=values, promised=promised)


# ---------------------------------------------------------------------------------------------------------------
def _neighbours(center_bits, offsets):
    """Bit patterns `offsets` ulps from a finite non-zero float32, kept where they stay finite, non-zero and of the
    same sign."""
    mag, sign = int(center_bits) & 0x7FFFFFFF, int(center_bits) & 0x80000000
    out = []
    for k in offsets:
        m = mag + k
        if 0 < m < 0x7F800000:
            out.append(sign | m)
    return out


ZERO_BAND_OFFSETS = sorted(set(list(range(-64, 65)) + [s * (1 << j) for j in range(7, 23) for s in (-1, 1)]))


def w_zero_ordinary(seed, shape="native", q33=0.37, n_rand_cols=2):
    """An ordinary rig WITHOUT CALIB_ZERO_DISPARITY, W = a d + b with b = q33 != 0 (the suite's 0.37 and -1/3): the
    float32 neighbours of -b / a, k ulps either side for k = 0..64 and 2^7 .. 2^22 ulps further out, laid down like
    the sweep.

    Built to reach: W changes sign inside the frame and cancels down to about a * ulp(d) ~ 2^-25 -- far above w_safe
    (~2^-116), so no pixel is a sliver pixel.  What it reaches is the cancellation in which the named forms round
    a * d and b + a * d apart while the default form rounds once (an accidental fma in a named form, or a split one
    in the default form, shows here and nowhere else), and the signs of the large results either side of the pole."""
    w, h, border, _ = SHAPES[shape]
    rng = np.random.default_rng((seed, 2, w, h))
    q = rig_q(w, h)
    q[15] = q33
    center = f32_bits(float(round_fraction_to_f32(-Fraction(float(q[15])) / Fraction(float(q[14])))))
    values = np.array(_neighbours(center, ZERO_BAND_OFFSETS), dtype=np.uint32)
    frames, placed, promised = _place(rng, _bits_to_f32(values), q, w, h, border, n_rand_cols)
    return SimpleNamespace(name="w_zero_ordinary", shape=shape, q=q, border=border, frames=frames, placed=placed,
                           values=values, promised=promised, d0=None)


SLIVER_D0 = np.float32(17.3)
# (a, focal length): a has one or two mantissa bits, so b = -a * d0 is exact; f = 713.5 is the reference rig, whose Z
# overflows before X and Y can; f = 2 lets |u + cx| and |v + cy| decide, by column and by row
SLIVER_RIGS = [(2.0 ** -120, None), (3 * 2.0 ** -121, None), (2.0 ** -120, 2.0)]


def w_zero_sliver(seed, shape="native", rig=0, sprinkle=0.15):
    """The sliver mix: a tiny a (SLIVER_RIGS) and b = -a * d0 for the float32 d0 = 17.3, exact in double, so that
    W = a (d - d0) exactly.  A plain k/8 frame with d0, its 2^j-ulp neighbours, and the float32 neighbours of the
    disparities at which the pixel's own X, Y or Z crosses the overflow threshold sprinkled over `sprinkle` of the ROI.

    Built to reach: W is exactly zero at d0, lies in the sliver 0 < |W| < w_safe for d within about 11 of d0 (a = 2^-120,
    f = 713.5: w_safe = f 2^-126) and is above w_safe further away, so that all three classes of the COMPACT kernels'
    predicate -- cheap accept, fall back to the real arithmetic, reject -- alternate inside one tile; with f ~ 714 Z
    overflows for |d - d0| < ~2.8, with f = 2 X and Y overflow at distances that depend on column and row: valid and
    invalid points interleave at single-ulp steps of d, which is where a count predicate and a store path that
    disagree by one point shift the rest of a COMPACT frame."""
    w, h, border, _ = SHAPES[shape]
    rng = np.random.default_rng((seed, 3, w, h, rig))
    a, f = SLIVER_RIGS[rig]
    q = rig_q(w, h) if f is None else rig_q(w, h, fx=f, fy=f)
    d0 = SLIVER_D0
    q[14] = a
    q[15] = -a * float(d0)
    assert Fraction(float(q[15])) == -Fraction(a) * Fraction(float(d0)), "b = -a * d0 must be exact"
    frames = _background(rng, 1, h, w)
    d0_bits = f32_bits(float(d0))
    near = _neighbours(d0_bits, [0] + [s * (1 << j) for j in range(0, 24) for s in (-1, 1)])
    # Z's overflow edge is the same for every pixel: |d - d0| = f / (a T)
    dz = Fraction(float(q[11])) / (Fraction(a) * OVERFLOW_THRESHOLD)
    for s in (-1, 1):
        c = f32_bits(float(round_fraction_to_f32(Fraction(float(d0)) + s * dz)))
        near += _neighbours(c, [-8, -2, -1, 0, 1, 2, 8])
    near = _bits_to_f32(near)
    rows, cols = np.nonzero(rng.random((h - 2 * border, w - 2 * border)) < sprinkle)
    rows, cols = rows + border, cols + border
    pick = rng.integers(0, len(near), size=len(rows))
    frames[0, rows, cols] = near[pick]
    placed = [(0, r, c, 0) for r, c in zip(rows, cols)]
    # X's and Y's own edges: five neighbouring disparities down one column whose |u + cx| exceeds every |v + cy| and f
    # (X overflows first there), and along one row whose |v + cy| exceeds the |u + cx| of the columns used and f
    fq, cxq, cyq = abs(float(q[11])), float(q[3]), float(q[7])
    k = 0
    for coord in (0, 1):
        for _ in range(24):
            r, c = int(rng.integers(border, h - border)), int(rng.integers(border, w - border))
            if coord == 0:
                num = abs(Fraction(c) + Fraction(cxq))
                line = [(int(rr), c) for rr in rng.permutation(np.arange(border, h - border))[:5]]
                if num <= max(fq, abs(border + cyq), abs(h - border - 1 + cyq)):
                    continue
            else:
                num = abs(Fraction(r) + Fraction(cyq))
                near_cols = [cc for cc in range(border, w - border) if abs(cc + cxq) < num]
                if num <= fq or len(near_cols) < 5:
                    continue
                line = [(r, int(cc)) for cc in rng.permutation(near_cols)[:5]]
            dd = Fraction(float(d0)) + (1 if k % 2 else -1) * num / (Fraction(a) * OVERFLOW_THRESHOLD)
            k += 1
            if not 0 < dd < 2 ** 100:
                continue
            nb = _neighbours(f32_bits(float(round_fraction_to_f32(dd))), [-2, -1, 0, 1, 2])
            for (rr, cc), bits in zip(line, nb):
                frames[0, rr, cc] = _bits_to_f32([bits])[0]
                placed.append((0, rr, cc, 1 + coord))
    return SimpleNamespace(name="w_zero_sliver", shape=shape, q=q, border=border, frames=frames,
                           placed=np.array(placed, dtype=np.int32), d0=d0, rig=rig)


def w_values(p):
    """W of every pixel of a w_zero pattern's frames in float64: a (d - d0), exact, for the sliver mix (the difference
    of two float32 is exact in double and a has at most two bits); fl(a d + b), good to 2^-53 |a d|, otherwise."""
    d = p.frames.astype(np.float64)
    if getattr(p, "d0", None) is not None:
        return float(p.q[14]) * (d - float(p.d0))
    return float(p.q[14]) * d + float(p.q[15])


# ---------------------------------------------------------------------------------------------------------------
EDGE_OFFSETS = [-8, -2, -1, 0, 1, 2, 8]
EDGES = {"overflow": Fraction(OVERFLOW_THRESHOLD), "min_normal": Fraction(1, 2 ** 126), "half_min_subnormal": Fraction(1, 2 ** 150)}


def edge_disparities(num, a, b, target):
    """The float32 disparities around the two d (one per sign of the quotient) at which |num / (a d + b)| equals
    `target` exactly (Fractions): bit patterns EDGE_OFFSETS ulps from the float32 nearest to each; none where that d is
    zero or beyond the finite float32 range."""
    out = []
    for s in (1, -1):
        d = (s * num / target - b) / a
        if d == 0 or abs(d) >= 2 ** 128 or abs(d) < Fraction(1, 2 ** 149):
            continue
        c = round_fraction_to_f32(d)
        if not np.isfinite(c) or c == 0:
            continue
        out.append(_neighbours(f32_bits(float(c)), EDGE_OFFSETS))
    return out


def overflow_edge(seed, shape="native", q=None):
    """For a stereo Q (default: the shape's reference rig) and for each of X, Y, Z in turn: the float32 disparities 0, 1,
    2 and 8 ulps either side of the d at which the pixel's exact quotient equals the float overflow threshold
    2^128 - 2^103, positive and negative, in a spread of columns (X: the principal pair, first, last, seeded) and rows
    (Y: the rows next to cy, first, last, seeded); the same for |X| = 2^-126 (the subnormal edge) and |X| = 2^-150
    (below which X rounds to zero), where a finite d reaches them.  Embedded in a k/8 frame.

    Built to reach: results whose exact value lies within an ulp of d of the threshold, where a reciprocal that is
    not correctly rounded, a product formed in float, or a finite test that disagrees with the store path returns
    FLT_MAX for inf or the reverse.  With the reference rig |u + cx| and |v + cy| are below f, so Z is already
    infinite where X and Y cross; the sliver mix with f = 2 is where they decide a point's validity.
    `placed` rows are (frame, row, col, group); `groups[g]` = (coordinate, edge name, sign)."""
    w, h, border, _ = SHAPES[shape]
    rng = np.random.default_rng((seed, 4, w, h))
    q = rig_q(w, h) if q is None else np.array(q, dtype=np.float64)
    a, b = Fraction(float(q[14])), Fraction(float(q[15]))
    frames = _background(rng, 1, h, w)
    used, placed, groups = set(), [], []

    def put(r, c, bits, g):
        assert (r, c) not in used
        used.add((r, c))
        frames[0, r, c] = _bits_to_f32([bits])[0]
        placed.append((0, r, c, g))

    def free_rows(c, n):
        rows = [r for r in rng.permutation(np.arange(border, h - border)).tolist() if (r, c) not in used]
        return rows[:n]

    def free_cols(r, n):
        cols = [c for c in rng.permutation(np.arange(border, w - border)).tolist() if (r, c) not in used]
        return cols[:n]

    pc = principal_cols(q, w, border)
    xcols = pc + [border, w - border - 1] + rng.choice(np.arange(border + 1, w - border - 1), 3, replace=False).tolist()
    above, below = _rows_by_side(q, h, border)
    yrows = [int(above[-1]), int(below[0]), border, h - border - 1] + rng.choice(np.arange(border + 1, h - border - 1), 3, replace=False).tolist()
    for c in dict.fromkeys(xcols):
        num = abs(Fraction(c) + Fraction(float(q[3])))
        for edge, target in EDGES.items():
            for vals in edge_disparities(num, a, b, target) if num else []:
                groups.append((0, edge, c))
                for r, bits in zip(free_rows(c, len(vals)), vals):
                    put(r, c, bits, len(groups) - 1)
    for r in dict.fromkeys(yrows):
        num = abs(Fraction(r) + Fraction(float(q[7])))
        for vals in edge_disparities(num, a, b, EDGES["overflow"]) if num else []:
            groups.append((1, "overflow", r))
            for c, bits in zip(free_cols(r, len(vals)), vals):
                put(r, c, bits, len(groups) - 1)
    for rep in range(4):
        for vals in edge_disparities(abs(Fraction(float(q[11]))), a, b, EDGES["overflow"]):
            groups.append((2, "overflow", rep))
            for bits in vals:
                r = int(rng.integers(border, h - border))
                put(r, free_cols(r, 1)[0], bits, len(groups) - 1)
    return SimpleNamespace(name="overflow_edge", shape=shape, q=q, border=border, frames=frames,
                           placed=np.array(placed, dtype=np.int32), groups=groups)


def near_integer_cx_q(shape="native"):
    """The shape's rig with its principal point 2^-21 left of a pixel centre: |u + cx| = 2^-21 in one column, small
    enough for |X| = 2^-150 to be reached by a finite d (the reference rig's 5e-4 is not)."""
    w, h, _, _ = SHAPES[shape]
    q = rig_q(w, h)
    q[3] = -(w // 2 - 2.0 ** -21)
    return q


# ---------------------------------------------------------------------------------------------------------------
def _f32(x):
    return float(np.float32(x))


# the reference's 1/8; mono16 seen as mono8 / 8; a full 24-bit mantissa; raw * scale subnormal for small raw values and
# normal for large ones; raw * scale = inf for large raw values
U16_SCALES = [0.125, float(np.float32(0.125) / np.float32(257)), _f32(0.37), _f32(1.37 * 2.0 ** -133), _f32(1e34)]
U8_SCALES = [0.125, float(np.float32(0.125) / np.float32(257)), _f32(0.37), _f32(1.37 * 2.0 ** -130), _f32(2e36)]


def _all_values(seed, shape, dtype):
    w, h, border, _ = SHAPES[shape]
    hi = int(np.iinfo(dtype).max) + 1
    rng = np.random.default_rng((seed, 5, w, h, hi))
    frame = rng.integers(0, hi, size=(h, w)).astype(dtype)
    rh, rw = h - 2 * border, w - 2 * border
    assert rh * rw >= hi
    spots = rng.permutation(rh * rw)[:hi]
    rows, cols = spots // rw + border, spots % rw + border
    frame[rows, cols] = np.arange(hi).astype(dtype)
    placed = np.stack([np.zeros(hi, np.int64), rows, cols, np.arange(hi)], axis=1).astype(np.int32)
    return frame[None], placed


def decode(raw, scale):
    """cvtScale as the kernels form it: float(raw) * float(scale), ONE fp32 rounding, subnormal products kept,
    overflow to inf."""
    with np.errstate(over="ignore", under="ignore"):
        return raw.astype(np.float32) * np.float32(scale)


def u16_all_values(seed, shape="native"):
    """Every 16-bit raw value at least once at seeded ROI positions, random values elsewhere; to be decoded with each of
    U16_SCALES.  Built to reach: the kernels' float(raw) * scale for all 65,536 inputs -- products that are exact
    (1/8), that round (0.37, 1/8/257), that are subnormal for small raw values and normal for large ones (a flushed
    subnormal product turns a finite or infinite point into NaN/inf of another sign), and that overflow to inf."""
    w, h, border, _ = SHAPES[shape]
    frames, placed = _all_values(seed, shape, np.uint16)
    return SimpleNamespace(name="u16_all_values", shape=shape, q=rig_q(w, h), border=border, frames=frames,
                           placed=placed, scales=U16_SCALES)


def u8_all_values(seed, shape="native"):
    """Every byte at least once at seeded ROI positions (U8_SCALES): as u16_all_values, and what the per-block
    256-entry tables of the fused callback kernels are indexed with."""
    w, h, border, _ = SHAPES[shape]
    frames, placed = _all_values(seed, shape, np.uint8)
    return SimpleNamespace(name="u8_all_values", shape=shape, q=rig_q(w, h), border=border, frames=frames,
                           placed=placed, scales=U8_SCALES)


def constant_cells(rng, h, w, border, k=3):
    """A random uint8 image whose ROI is tiled with k x k cells of one value each, the values running through all 256
    bytes in a seeded order: a k x k median is the identity at the cell centres, so every byte reaches the
    reprojection through the filter.  -> (image, mask of the cell centres)."""
    img = rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    centre = np.zeros((h, w), dtype=bool)
    r = k // 2
    ys, xs = np.arange(border + r, h - border - r, k), np.arange(border + r, w - border - r, k)
    vals = (rng.permutation(len(ys) * len(xs)) % 256).astype(np.uint8).reshape(len(ys), len(xs))
    for i, y in enumerate(ys):
        for j, x in enumerate(xs):
            img[y - r:y + r + 1, x - r:x + r + 1] = vals[i, j]
    centre[np.ix_(ys, xs)] = True
    return img, centre


FLOAT_PATTERNS = ["binade_sweep", "w_zero_ordinary_0.37", "w_zero_ordinary_-1/3", "w_zero_sliver_0", "w_zero_sliver_1",
                  "w_zero_sliver_2", "overflow_edge", "overflow_edge_near_integer_cx"]


def make(name, shape, seed=7):
    """One of FLOAT_PATTERNS at one of SHAPES."""
    if name == "binade_sweep":
        return binade_sweep(seed, shape)
    if name.startswith("w_zero_ordinary_"):
        q33 = {"0.37": 0.37, "-1/3": -1.0 / 3.0}[name[len("w_zero_ordinary_"):]]
        return w_zero_ordinary(seed, shape, q33)
    if name.startswith("w_zero_sliver_"):
        return w_zero_sliver(seed, shape, int(name[-1]))
    if name == "overflow_edge":
        return overflow_edge(seed, shape)
    if name == "overflow_edge_near_integer_cx":
        return overflow_edge(seed, shape, near_integer_cx_q(shape))
    raise KeyError(name)


_cache = {}


def with_exact(name, shape, seed=7):
    """make(name, shape) with its exact answers (exact_reproject) as `.exact`; computed once per process."""
    from exact_reproject import exact_reproject
    key = (name, shape, seed)
    if key not in _cache:
        p = make(name, shape, seed)
        p.exact = exact_reproject(p.q, p.frames, p.border)
        _cache[key] = p
    return _cache[key]


BIT_EQUAL_DIST = 2.0 ** -45   # farther than this (relative) from a rounding boundary: the default form must hit the exact bits


def bit_equal_mask(exact):
    """Points whose three coordinates all lie farther than BIT_EQUAL_DIST from a float32 rounding boundary."""
    return exact["has_exact"] & (exact["dist"] > BIT_EQUAL_DIST).all(axis=-1)
