"""Seeded value distributions for the device median and the fused callback kernels (numpy only).

iid uniform bytes -- what most of the suite feeds -- give k = 11 medians between about 65 and 185 and bit-plane
counts near k^2 / 2, so they never read the high and low entries of the per-byte tables and never drive the
select's counts towards 0 or k^2.  Each generator below says what it is built to reach; tests/test_value_patterns.py
checks that it does, at the shapes the GPU tests use.
"""
import numpy as np

TILE_W, TILE_H = 256, 32   # the bit-sliced median's tile (d2pc_median_bs_tile.hpp)

# (lo, hi) pairs of two_level: (127, 128) differ in every bit plane, the peeled MSB one included; (0, 1) and
# (254, 255) only in the LSB; the others at plane boundaries and across the range.
TWO_LEVEL_PAIRS = [(127, 128), (0, 1), (254, 255), (63, 64), (191, 192), (0, 255), (85, 170), (128, 129)]
# (lo, width) of narrow_band: the bottom and top of the table, the middle, a plane boundary, wider ends.
NARROW_BANDS = [(0, 4), (252, 4), (126, 4), (60, 8), (0, 16), (240, 16)]


def window_counts(mask: np.ndarray, k: int) -> np.ndarray:
    """k x k box sum of a 0/1 mask with a replicated border (cv::medianBlur's border): the number of set pixels in
    the window of every pixel."""
    r = k // 2
    m = np.pad(np.asarray(mask, dtype=np.int32), r, mode="edge")
    c = np.cumsum(np.cumsum(m, axis=0), axis=1)
    c = np.pad(c, ((1, 0), (1, 0)))
    h, w = mask.shape
    return c[k:k + h, k:k + w] - c[:h, k:k + w] - c[k:k + h, :w] + c[:h, :w]


def two_level(rng, h, w, lo, hi, k=11):
    """Each pixel is `hi` with a probability that rises from 0 (top rows) to 1 (bottom rows), else `lo`.  Built to
    reach: the number of `hi` pixels in a k x k window takes every value 0..k^2 and crosses the rank k^2 // 2 in
    every column, so at the bit plane where lo and hi part, the select's count runs through its whole range and
    the median flips between lo and hi.  The ramp is flat for k // 2 + 1 rows at either end so that the windows
    of the first and last rows are pure."""
    pad = k // 2 + 1
    p = np.clip((np.arange(h, dtype=np.float64) - pad + 0.5) / max(h - 2 * pad, 1), 0.0, 1.0)
    hit = rng.random((h, w)) < p[:, None]
    return np.where(hit, np.uint8(hi), np.uint8(lo)).astype(np.uint8)


def two_level_tiles(rng, h, w, lo, hi):
    """`hi` with a density of its own in every 256 x 32 tile of the image, the densities spread evenly over
    [0, 1] in a random order.  Built to reach: within one tile of the bit-sliced median every lane sees about the
    same count, near 0 or k^2 in some tiles and at the rank boundary in others; across tile edges the counts
    jump."""
    ty, tx = -(-h // TILE_H), -(-w // TILE_W)
    dens = rng.permutation(np.linspace(0.0, 1.0, ty * tx)).reshape(ty, tx)
    p = np.repeat(np.repeat(dens, TILE_H, axis=0), TILE_W, axis=1)[:h, :w]
    return np.where(rng.random((h, w)) < p, np.uint8(hi), np.uint8(lo)).astype(np.uint8)


def narrow_band(rng, h, w, lo, width):
    """Uniform in [lo, lo + width).  Built to reach: every median lies in the band, so at the top or bottom of the
    byte range the high planes are constant and the select decides on the low bits only."""
    return rng.integers(lo, lo + width, size=(h, w)).astype(np.uint8)


def _tri(phase):
    """Triangle wave over one unit of phase, clipped into plateaus at 0 and 255 (about an eighth of a period each):
    a plateau wider than the window keeps its value through the median."""
    t = 1.0 - np.abs(2.0 * (phase - np.floor(phase)) - 1.0)
    return np.clip((t - 0.12) / 0.76, 0.0, 1.0) * 255.0


def scene_pieces(rng, h, w):
    """The planes of smooth_scene: vertical strips (x0, x1, gx, gy, c) -- in each, value = tri(gx*x + gy*y + c).
    Strip edges are occlusion steps.  The period along x is about a third of the width (at least 72 pixels), so a
    strip covers one to two ramps; its phase offset is random."""
    period = max(w / 3.0, 72.0)
    edges = [0]
    while edges[-1] < w:
        edges.append(edges[-1] + int(rng.integers(int(period * 0.6), int(period * 1.4) + 1)))
    edges[-1] = w
    pieces = []
    for x0, x1 in zip(edges[:-1], edges[1:]):
        gx = rng.choice([-1.0, 1.0]) * rng.uniform(0.8, 1.25) / period
        gy = rng.uniform(-0.5, 0.5) / period
        pieces.append((x0, x1, gx, gy, rng.random()))
    return pieces


def render_scene(pieces, h, w):
    """The noise-free scene of `pieces` as float64 values in [0, 255]."""
    out = np.empty((h, w), dtype=np.float64)
    y = np.arange(h, dtype=np.float64)[:, None]
    for x0, x1, gx, gy, c in pieces:
        x = np.arange(x0, x1, dtype=np.float64)[None, :]
        out[:, x0:x1] = _tri(gx * x + gy * y + c)
    return out


def hole_mask(rng, h, w, frac=0.3, block=32):
    """About `frac` of the image in zero blocks of block x block pixels (regions without a stereo match)."""
    m = rng.random((-(-h // block), -(-w // block))) < frac
    return np.repeat(np.repeat(m, block, axis=0), block, axis=1)[:h, :w]


def smooth_scene(rng, h, w, holes=False, impulses=False):
    """Piecewise-planar disparity like a real stereo map: slanted planes with a clipped triangle-wave profile
    (scene_pieces), +-2 noise, occlusion steps between the planes; with `holes` about 30 % blocky zero holes,
    with `impulses` sparse 0 / 255 outliers (0.5 %).  Built to reach: inside the ROI (border 40 at 752 x 480 and
    larger, border 7 at small shapes) the k = 11 median takes all 256 byte values, so every entry of the
    per-byte tables is read, and zero holes give byte-0 points (NaN / inf)."""
    v = render_scene(scene_pieces(rng, h, w), h, w) + rng.integers(-2, 3, size=(h, w))
    img = np.clip(np.rint(v), 0, 255).astype(np.uint8)
    if holes:
        img[hole_mask(rng, h, w)] = 0
    if impulses:
        spot = rng.random((h, w)) < 0.005
        img[spot] = np.where(rng.random(int(spot.sum())) < 0.5, 0, 255).astype(np.uint8)
    return img


def roi_values(img: np.ndarray, border: int) -> np.ndarray:
    """The distinct byte values of `img` inside the ROI inset by `border`."""
    h, w = img.shape
    return np.unique(img[border:h - border, border:w - border])


def two_level_frames(seed, h, w, k=11):
    """One frame per pair of TWO_LEVEL_PAIRS, the row ramp (two_level) and the per-tile densities (two_level_tiles)
    taking turns (seeds of the other parity swap them): -> list of (image, lo, hi)."""
    out = []
    for i, (lo, hi) in enumerate(TWO_LEVEL_PAIRS):
        rng = np.random.default_rng((seed, i))
        img = two_level(rng, h, w, lo, hi, k) if (i + seed) % 2 == 0 else two_level_tiles(rng, h, w, lo, hi)
        out.append((img, lo, hi))
    return out


def smooth_frames(seed, n, h, w):
    """n smooth scenes; every second one with zero holes and impulses once the image is large enough for blocks of
    32 to leave planes between them (at least 128 x 128)."""
    big = h >= 128 and w >= 128
    return [smooth_scene(np.random.default_rng((seed, i)), h, w, holes=big and i % 2 == 1, impulses=big and i % 2 == 1)
            for i in range(n)]
