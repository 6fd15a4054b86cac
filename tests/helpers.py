"""Shared helpers for the parity tests (numpy only)."""
import numpy as np



def variant_for(algo=0, pxt=8, exp=False):
    """Which build a test loads: the product libd2pc.so (None) or the experiment build of `make exp`, libd2pc_exp.so
    ("exp").  compact_algo 4 (the chunked two-pass), tile shapes other than 2,048 pixels, the tile-walking PARITY kernel
    and round 2's fused general-Q form exist only in the latter (include/d2pc_ext.h, "experiment build")."""
    return "exp" if (algo == 4 or pxt != 8 or exp) else None


DEFAULT_CALIB = dict(fx=714.24, fy=713.5, cx=376.0, cy=240.0, baseline=0.09, nx=752, ny=480)


def line_bits(x):
    """float32 values (or their uint32 bit patterns) on a monotone integer line: the position of a finite float is its
    magnitude's bit pattern, negated for negative values, so that neighbouring floats are 1 apart and +-inf is the
    position after +-FLT_MAX.  NaN has no meaningful position (callers mask it)."""
    b = np.asarray(x)
    b = (np.ascontiguousarray(b).view(np.uint32) if b.dtype == np.float32 else b.astype(np.uint32)).astype(np.int64)
    mag = b & 0x7FFFFFFF
    return np.where(b & 0x80000000 != 0, -mag, mag)


def ulp_distance(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Distance in float32 ulps between finite values (0 when both are the
    same inf or both NaN; a huge number when the classes differ)."""
    a = np.ascontiguousarray(a, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    # map the sign-magnitude float ordering onto a monotone integer line
    ai, bi = line_bits(a), line_bits(b)
    d = np.abs(ai - bi)
    both_nan = np.isnan(a) & np.isnan(b)
    one_nan = np.isnan(a) ^ np.isnan(b)
    d = np.where(both_nan, 0, d)
    d = np.where(one_nan, 1 << 40, d)
    return d


def assert_points_close(got: np.ndarray, want: np.ndarray, max_ulp=2, rel=1e-5, what=""):
    """The parity bar for XYZ: identical NaN/inf classes, pad word bit-exact,
    finite values within `rel` relative (BASELINE.json north_star: 1e-5) and,
    tighter, within `max_ulp` float32 ulps."""
    got = np.asarray(got, dtype=np.float32).reshape(-1, 4)
    want = np.asarray(want, dtype=np.float32).reshape(-1, 4)
    assert got.shape == want.shape, f"{what}: shape {got.shape} vs {want.shape}"
    assert np.array_equal(got[:, 3].view(np.uint32), want[:, 3].view(np.uint32)), f"{what}: pad word"
    g, w = got[:, :3], want[:, :3]
    assert np.array_equal(np.isnan(g), np.isnan(w)), f"{what}: NaN positions differ"
    assert np.array_equal(np.isposinf(g), np.isposinf(w)), f"{what}: +inf positions differ"
    assert np.array_equal(np.isneginf(g), np.isneginf(w)), f"{what}: -inf positions differ"
    fin = np.isfinite(w)
    if fin.any():
        gw, ww = g[fin].astype(np.float64), w[fin].astype(np.float64)
        denom = np.maximum(np.abs(ww), np.finfo(np.float32).tiny)
        relerr = np.abs(gw - ww) / denom
        assert relerr.max() <= rel, f"{what}: max rel err {relerr.max():.3e} > {rel}"
        d = ulp_distance(g[fin], w[fin])
        assert d.max() <= max_ulp, f"{what}: max ulp distance {d.max()} > {max_ulp}"


from disparity_to_point_cloud_amd.synth import frame_seed, synth_disparity  # noqa: E402,F401
