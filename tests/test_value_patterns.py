"""The value patterns of tests/value_patterns.py reach what they are built to reach, at the shapes and seeds the GPU
tests (test_median_values_gpu.py) use; and the oracle's two medians are pinned to scipy on them."""
import numpy as np
import pytest

import oracle
import value_patterns as vp

GPU_SHAPES = [(752, 480), (520, 261), (257, 33)]   # (w, h)
SMOOTH_ROIS = [(752, 480, 40), (520, 261, 40), (520, 261, 7), (257, 33, 7)]   # (w, h, border)
SMOOTH_SEEDS = range(4)


def test_window_counts_is_the_replicated_border_box_sum():
    rng = np.random.default_rng(0)
    m = rng.random((23, 17)) < 0.4
    for k in (3, 5, 11):
        r = k // 2
        p = np.pad(m.astype(np.int64), r, mode="edge")
        want = np.array([[p[y:y + k, x:x + k].sum() for x in range(17)] for y in range(23)])
        assert np.array_equal(vp.window_counts(m, k), want)


@pytest.mark.parametrize("w,h", GPU_SHAPES)
@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
def test_two_level_window_counts_take_every_value(k, w, h):
    """The number of `hi` pixels in a window runs through 0..k^2 (so the select's count at the plane where lo and hi
    part does too); the per-tile form as well wherever the image holds enough tiles for its density steps."""
    for seed in (0, 1):
        for i, (img, lo, hi) in enumerate(vp.two_level_frames(seed, h, w, k)):
            tiles = (i + seed) % 2 == 1
            if tiles and -(-h // vp.TILE_H) * -(-w // vp.TILE_W) < 12:
                continue
            c = vp.window_counts(img == hi, k)
            assert set(np.unique(c).tolist()) == set(range(k * k + 1)), (seed, lo, hi, tiles)
            assert set(np.unique(img).tolist()) == {lo, hi}


@pytest.mark.parametrize("w,h,border", SMOOTH_ROIS)
def test_smooth_scene_median_takes_every_byte_value_inside_the_roi(w, h, border):
    for seed in SMOOTH_SEEDS:
        for i, img in enumerate(vp.smooth_frames(seed, 4, h, w)):
            got = vp.roi_values(oracle.median_u8(img, 11), border)
            assert len(got) == 256, (seed, i, sorted(set(range(256)) - set(got.tolist()))[:8])


def test_smooth_scene_holes_and_impulses():
    """The holey scenes carry about 30 % zeros in blocks, and impulses of both extremes."""
    img = vp.smooth_scene(np.random.default_rng(5), 480, 752, holes=True, impulses=True)
    plain = vp.smooth_scene(np.random.default_rng(5), 480, 752)
    zero = (img == 0) & (plain != 0)
    assert 0.2 < zero.mean() < 0.4
    assert ((img == 255) & (plain < 250)).sum() > 100


def test_smooth_scene_median_takes_every_byte_value_at_4k():
    rng = np.random.default_rng(7)
    for holes in (False, True):
        img = vp.smooth_scene(rng, 2160, 3840, holes=holes, impulses=holes)
        assert len(vp.roi_values(oracle.median_u8_fast(img, 11), 40)) == 256, holes


@pytest.mark.parametrize("lo,width", vp.NARROW_BANDS)
def test_narrow_band_medians_stay_in_the_band(lo, width):
    img = vp.narrow_band(np.random.default_rng(lo + width), 261, 520, lo, width)
    assert img.min() == lo and img.max() == lo + width - 1
    for k in (3, 11):
        m = oracle.median_u8(img, k)
        assert lo <= m.min() and m.max() < lo + width


def _small_frames(h, w):
    out = [img for img, _, _ in vp.two_level_frames(3, h, w, 5)]
    out += [vp.narrow_band(np.random.default_rng(i), h, w, lo, width) for i, (lo, width) in enumerate(vp.NARROW_BANDS)]
    out += vp.smooth_frames(3, 2, h, w)
    return out


@pytest.mark.parametrize("w,h", [(67, 45), (33, 7), (130, 131), (5, 3)])
@pytest.mark.parametrize("k", [3, 5, 11])
def test_both_oracle_medians_equal_scipy_on_the_value_patterns(k, w, h):
    ndimage = pytest.importorskip("scipy.ndimage")
    for img in _small_frames(h, w):
        want = ndimage.median_filter(img, size=k, mode="nearest")
        assert np.array_equal(oracle.median_u8(img, k), want)
        assert np.array_equal(oracle.median_u8_fast(img, k), want)
        view = np.pad(img, ((0, 0), (0, 9)))[:, :w]   # strided rows
        assert np.array_equal(oracle.median_u8_fast(view, k), want)
