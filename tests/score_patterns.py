"""Inputs that take the matching-score pre-filter where uniform bytes and noisy blocks do not,
and a restatement of the chain with one slip at a time.

Random frames blur to a nearly flat A: five G13 rounding ties per camera frame and none that moves an I across the
threshold, B below 178, A below 243.  The generators here are seeded, return (frame, square), and each is built to reach
one thing; tests/test_score_patterns.py asserts the reach at the shapes and seeds the GPU tests use.

  planted_ties      G13 sums of exactly 65536 q + 32768 on a grid of disjoint windows (pitch 14: every distance from a
                    32- and a 64-pixel tile seam occurs), odd and even q alternating, on valleys whose I sits just
                    under the threshold, so that rounding a tie the other way moves an M
  threshold_band    parabolic valleys c p^2 along the derivative axis: the integer Sobel of c p^2 is 2048 c, c is taken
                    round 1017 / 2048 per valley; every third valley is steep enough for a full 21 x 21 window of ones
  b_extremes        the same valleys with c ramping ALONG the valley from 0.42 to 0.62: the density of M goes from 0 to
                    1 and B through every value up to the form's maximum, next to small and large S
  a_extremes        24 x 24 cells of 0 and 255: A = 253 and 0, H = 65,025, the largest |I| of both signs
  frame_vs_square   cells of 5 x 5 random bytes; the square strictly inside, so that what lies outside it contradicts
                    the mirror image of the inside

The left half of every valley frame has its derivative axis along y (direction 0 fires there), the right half along x.

stages_mutant(frame, square, direction, form, mutant) is score_filter_ref.stages rebuilt from the same pieces with the
switches of MUTANTS; mutant None is the spec.  "b_round_swap" (CV4's B rounded half to even, CV3's half up) is listed
in UNKILLABLE: 255 s = 32768 (mod 65536) forces s = 32768 (255 is invertible), where q = 127 is odd and both rules give
128 -- no input tells the two apart (test_score_patterns.py enumerates it), so nobody needs to build a pattern for it."""
import itertools

import numpy as np

import score_filter_ref as ref

MUTANTS = (
    "a_half_up", "a_trunc", "thr_1016", "thr_1018", "g13_about_square", "post_about_frame",
    "g13_border_reflect", "sobel_border_reflect", "g21_border_reflect", "dir_swap", "other_t21", "b_trunc",
    "out_wrap", "out_sat254", "grad_sat",
)
UNKILLABLE = ("b_round_swap",)

CAMERA = ((480, 752), (133, 15, 465))   # the fusion node's frame and square (offsets -7 / 15)
RAGGED = ((190, 203), (17, 9, 171))     # n = 5 * 32 + 11 = 2 * 64 + 43


# ---- the chain with one slip -------------------------------------------------------------------------------------
def _border(idx, length, kind):
    """borderInterpolate: kind 101 = BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), 1 = BORDER_REFLECT (fedcba|abcdefgh|hgfedcb)."""
    if kind == 101:
        return ref.refl(idx, length)
    idx = np.asarray(idx, np.int64)
    p = np.mod(idx, 2 * length)
    return np.where(p < length, p, 2 * length - 1 - p)


def _pad(img, r, kind=101):
    rows = _border(np.arange(-r, img.shape[0] + r), img.shape[0], kind)
    cols = _border(np.arange(-r, img.shape[1] + r), img.shape[1], kind)
    return img[np.ix_(rows, cols)]


def stages_mutant(frame, square, direction, form=4, mutant=None):
    """dict with A, I, M (0/1), B, out, grad of one frame under `mutant` (None: the spec, equal to ref.stages)."""
    assert mutant is None or mutant in MUTANTS or mutant in UNKILLABLE, mutant
    frame = np.asarray(frame)
    assert frame.dtype == np.uint8 and frame.ndim == 2
    x, y, n = square
    h, w = frame.shape
    t13, t21 = ref.tap_tables(form)
    if mutant == "other_t21":
        t21 = ref.tap_tables(7 - form)[1]
    if mutant == "dir_swap":
        direction ^= 1
    whole = mutant == "post_about_frame"  # filter the whole frame, crop at the end
    if whole:
        src = _pad(frame.astype(np.int64), 6)
    elif mutant == "g13_about_square":
        i = ref.refl(np.arange(-6, n + 6), n)
        src = frame[np.ix_(y + i, x + i)].astype(np.int64)
    else:
        k13 = 1 if mutant == "g13_border_reflect" else 101
        rows = _border(y + np.arange(-6, n + 6), h, k13)
        cols = _border(x + np.arange(-6, n + 6), w, k13)
        src = frame[np.ix_(rows, cols)].astype(np.int64)
    s13 = ref._sep(src, t13, t13)
    if mutant == "a_half_up":
        a = (s13 + 0x8000) >> 16
    elif mutant == "a_trunc":
        a = s13 >> 16
    else:
        a = ref.rint_even_16(s13)
    kr, kc = (ref.SOBEL_S, ref.SOBEL_D) if direction == 0 else (ref.SOBEL_D, ref.SOBEL_S)
    i = ref._sep(_pad(a, 3, 1 if mutant == "sobel_border_reflect" else 101), kr, kc)
    m = (i >= {"thr_1016": 1016, "thr_1018": 1018}.get(mutant, ref.THRESHOLD_I)).astype(np.int64)
    v = 255 * ref._sep(_pad(m, 10, 1 if mutant == "g21_border_reflect" else 101), t21, t21)
    half_up = (form == 4) != (mutant == "b_round_swap")
    b = v >> 16 if mutant == "b_trunc" else (v + 0x8000) >> 16 if half_up else ref.rint_even_16(v)
    if whole:
        a, i, m, b = (p[y:y + n, x:x + n] for p in (a, i, m, b))
    s = frame[y:y + n, x:x + n].astype(np.int64)
    t = s + 2 * b
    out = t & 255 if mutant == "out_wrap" else np.minimum(254 if mutant == "out_sat254" else 255, t)
    grad = np.minimum(255, t) if mutant == "grad_sat" else b
    return {"A": a, "I": i, "M": m, "B": b, "out": out.astype(np.uint8), "grad": grad.astype(np.uint8)}


def row_sums(frame, square, direction):
    """The kernel's 16-bit intermediates: H (G13 along rows: uint16 on the device), P (Sobel along rows of A: int16)."""
    x, y, n = square
    h, w = frame.shape
    t13, _ = ref.tap_tables(4)
    rows = ref.refl(y + np.arange(-6, n + 6), h)
    cols = ref.refl(x + np.arange(-6, n + 6), w)
    one = np.array([1], np.int64)
    hh = ref._sep(frame[np.ix_(rows, cols)].astype(np.int64), t13, one)
    a = ref.rint_even_16(ref._sep(hh, one, t13))
    p = ref._sep(_pad(a, 3)[3:-3], ref.SOBEL_S if direction == 0 else ref.SOBEL_D, one)
    return hh, p


def b_max(form):
    """The largest B of a form, from its tap sums: a 21 x 21 window of ones."""
    t = int(ref.tap_tables(form)[1].sum())
    v = 255 * t * t
    return (v + 0x8000) >> 16 if form == 4 else int(ref.rint_even_16(v))


# ---- valleys -----------------------------------------------------------------------------------------------------
def _valleys(length, width, period, off, coef, rng, noise):
    """length x width bytes: off + c p^2 along axis 0, p the distance from the valley's centre line, c = coef(valley
    index array, width) -> (valleys x width)."""
    r = np.arange(length)
    k = r // period
    p = (r % period) - period // 2
    c = coef(int(k.max()) + 1, width)
    f = off + c[k, :] * (p * p)[:, None].astype(np.float64)
    f = np.rint(f) + rng.integers(-noise, noise + 1, size=f.shape)
    return np.clip(f, 0, 255).astype(np.uint8)


def _two_regions(shape, square, period, off, coef, rng, noise):
    """Left of the square's middle column: valleys along x with the derivative axis y; right of it: transposed."""
    h, w = shape
    mid = square[0] + square[2] // 2
    f = np.empty(shape, np.uint8)
    f[:, :mid] = _valleys(h, mid, period, off, coef, rng, noise)
    f[:, mid:] = _valleys(w - mid, h, period, off, coef, rng, noise).T
    return f


def threshold_band(shape=CAMERA[0], square=CAMERA[1], seed=2):
    rng = np.random.default_rng(seed)
    c0 = ref.THRESHOLD_I / 2048.0

    def coef(nv, width):
        c = c0 + rng.uniform(-0.003, 0.003, size=nv)[:, None] + np.linspace(-0.003, 0.003, width)[None, :]
        c[1::3] = 0.60  # steep valleys: I clear of the threshold, a block of ones wider than 21
        return c

    return _two_regions(shape, square, 48, 0, coef, rng, 1), tuple(square)


def b_extremes(shape=CAMERA[0], square=CAMERA[1], seed=3):
    rng = np.random.default_rng(seed)

    def coef(nv, width):
        ramp = np.linspace(0.42, 0.62, width)
        c = np.repeat(ramp[None, :], nv, axis=0)
        c[1::2] = c[1::2, ::-1]  # neighbouring valleys ramp opposite ways
        return c

    return _two_regions(shape, square, 48, 0, coef, rng, 1), tuple(square)


# ---- planted ties ------------------------------------------------------------------------------------------------
TIE_PITCH = 14  # > 13: disjoint G13 windows; coprime to 32 / 2: every odd distance from a tile seam occurs


def _fine_table():
    """r -> (d, e, f) with 25 d + 45 e + 81 f = r (the window's corner weights t13[0]^2, t13[0] t13[1], t13[1]^2), the
    smallest max |.| first."""
    t = {}
    rng_ = range(-12, 13)
    for d, e, f in sorted(itertools.product(rng_, rng_, rng_), key=lambda v: (max(map(abs, v)), sum(map(abs, v)))):
        t.setdefault(25 * d + 45 * e + 81 * f, (d, e, f))
    return t


_FINE = None


def _plant(f, fy, fx, parity, k):
    """Nudge a few pixels of the 13 x 13 window of frame pixel (fy, fx) until its exact G13 sum is 65536 q + 32768
    with q of the given parity.  False (frame untouched) when a pixel would leave 0..255."""
    global _FINE
    if _FINE is None:
        _FINE = _fine_table()
    win = f[fy - 6:fy + 7, fx - 6:fx + 7].astype(np.int64)
    s0 = int((k * win).sum())
    d = (0x8000 + 0x10000 * parity - s0) % 0x20000
    if d > 0x10000:
        d -= 0x20000
    ring = int(k[5:8, 5:8].sum())  # the centre 3 x 3
    a9 = int(np.rint(d / ring))
    d -= a9 * ring
    a1 = int(np.rint(d / int(k[6, 6])))
    d -= a1 * int(k[6, 6])
    if d not in _FINE:
        return False
    win[5:8, 5:8] += a9
    win[6, 6] += a1
    win[0, 0], win[0, 1], win[1, 1] = win[0, 0] + _FINE[d][0], win[0, 1] + _FINE[d][1], win[1, 1] + _FINE[d][2]
    if win.min() < 0 or win.max() > 255:
        return False
    assert int((k * win).sum()) % 0x20000 == 0x8000 + 0x10000 * parity
    f[fy - 6:fy + 7, fx - 6:fx + 7] = win
    return True


def plant_ties(frame, square, sites=None):
    """Plant ties in place at square pixels (r, c) of `sites` (default: the pitch-14 grid from 7, 7) whose window lies
    inside the frame; q parity alternates like a chessboard over the grid.  Returns the planted (r, c, parity)."""
    x, y, n = square
    h, w = frame.shape
    t13 = ref.tap_tables(4)[0]
    k = np.outer(t13, t13)
    if sites is None:
        g = range(7, n, TIE_PITCH)
        sites = [(r, c, ((r + c) // TIE_PITCH) & 1) for r in g for c in g]
    f = frame.astype(np.int64)
    done = []
    for r, c, par in sites:
        fy, fx = y + r, x + c
        if fy - 6 < 0 or fx - 6 < 0 or fy + 6 >= h or fx + 6 >= w:
            continue
        if _plant(f, fy, fx, par, k):
            done.append((r, c, par))
    frame[...] = f.astype(np.uint8)
    return done


def planted_ties(shape=CAMERA[0], square=CAMERA[1], seed=1):
    rng = np.random.default_rng(seed)

    def coef(nv, width):  # 2048 c = 1017 - 55 .. 1017 - 15: a sparse M, so that S + 2 B stays below 255 near the sites
        return np.repeat(rng.uniform(0.470, 0.489, size=nv)[:, None], width, axis=1)

    f = _two_regions(shape, square, 40, 64, coef, rng, 2)
    plant_ties(f, square)
    return f, tuple(square)


def tie_sites(frame, square):
    """(r, c, q) of every square pixel whose exact G13 sum is 65536 q + 32768."""
    x, y, n = square
    h, w = frame.shape
    t13 = ref.tap_tables(4)[0]
    rows = ref.refl(y + np.arange(-6, n + 6), h)
    cols = ref.refl(x + np.arange(-6, n + 6), w)
    s = ref._sep(frame[np.ix_(rows, cols)].astype(np.int64), t13, t13)
    r, c = np.nonzero((s & 0xFFFF) == 0x8000)
    return r, c, s[r, c] >> 16


# ---- blocks ------------------------------------------------------------------------------------------------------
def a_extremes(shape=CAMERA[0], square=CAMERA[1], seed=4):
    """24 x 24 cells of 0 / 255 (wider than the 19 pixels G13 and the Sobel need for a constant window), the grid 5 off
    the frame's origin so that cell and tile edges do not coincide."""
    rng = np.random.default_rng(seed)
    h, w = shape
    cells = rng.integers(0, 2, size=(h // 24 + 2, w // 24 + 2)).astype(np.uint8) * 255
    return np.kron(cells, np.ones((24, 24), np.uint8))[5:5 + h, 5:5 + w].copy(), tuple(square)


def frame_vs_square(shape=CAMERA[0], corner="tl", inset=3, seed=5):
    """Cells of 5 x 5 random bytes.  The square sits `inset` pixels (1..6: G13 reflects about the frame for part of
    its reach) from the two frame edges of `corner` (tl / br) and at least 7 from the other two."""
    rng = np.random.default_rng(seed)
    h, w = shape
    cells = rng.integers(0, 256, size=(h // 5 + 2, w // 5 + 2)).astype(np.uint8)
    f = np.kron(cells, np.ones((5, 5), np.uint8))[2:2 + h, 2:2 + w].copy()  # (every reach of 6 crosses a cell edge)
    n = min(h, w) - inset - 7
    sq = (inset, inset, n) if corner == "tl" else (w - n - inset, h - n - inset, n)
    return f, sq


PATTERNS = {
    "planted_ties": planted_ties, "threshold_band": threshold_band, "b_extremes": b_extremes, "a_extremes": a_extremes,
    "frame_vs_square": lambda shape=CAMERA[0], square=None, seed=5: frame_vs_square(shape, "tl", 3, seed),
}


def pattern(name, which="camera"):
    """(frame, square) of a named pattern at the camera or the ragged shape."""
    shape, square = CAMERA if which == "camera" else RAGGED
    return PATTERNS[name](shape, square)


def golden_crops():
    """(name, frame, square) of a 45 x 45 crop of each camera-shaped pattern with the square (6, 6, 33) inside: small
    enough for the exact-rational chain of tests/golden/make_score_filter_golden.py (stored in score_filter.npz)."""
    at = {"planted_ties": (78, 200), "planted_ties_t": (100, 443), "threshold_band": (100, 200), "threshold_band_t": (100, 463),
          "b_extremes": (100, 250), "b_extremes_t": (250, 463), "a_extremes": (60, 300), "frame_vs_square": (0, 0)}
    for name, (r0, c0) in at.items():  # (_t: from the right half, where direction 1 fires)
        f, _ = pattern(name[:-2] if name.endswith("_t") else name, "camera")
        yield f"pat_{name}", np.ascontiguousarray(f[r0:r0 + 45, c0:c0 + 45]), (6, 6, 33)
