"""Shared helpers for the parity tests (numpy only; the two device helpers at the end import torch when called)."""
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


def run_batch(ctx, frames, want_index=True, scale=1.0):
    """All frames in one launch of d2pc_process_device -> (points (n, stride, 4), index (n, stride) or None, counts)."""
    import torch
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    n, (h, w) = len(frames), frames[0].shape
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}[frames[0].dtype]
    b = DeviceBatch(ctx, n, h, w, dtype=tdt, want_index=want_index)
    stack = np.stack(frames)
    b.disp.copy_(torch.from_numpy(stack.view(np.int16)).view(tdt) if stack.dtype == np.uint16 else torch.from_numpy(stack))
    b.points.fill_(float("nan"))
    b.counts.fill_(-7)
    b.launch(scale=scale)
    torch.cuda.synchronize()
    ctx.check_async_error()
    counts = b.counts.cpu().numpy().view(np.uint32).copy()
    pts = b.points.cpu().numpy()
    idx = b.index.cpu().numpy().view(np.uint32) if want_index else None
    return pts, idx, counts, b.roi_n


def check_compact_is_filtered_parity(ctx, algo, frames, dmin, want_index, what, scale=1.0, decoded=None):
    """Points, indices and counts of a COMPACT launch against the SAME context's PARITY launch filtered on the host by
    isfinite(X) & isfinite(Y) & isfinite(Z) & !(d <= min_disparity), in order -- exactly what the w_safe shortcut of
    the count predicates promises, and no oracle involved.  The COMPACT launch must have been served by `algo`: the
    single pass (2) and the resident blocks (3) count their launches, a re-route to the two-pass form does not."""
    import disparity_to_point_cloud_amd as d2pc
    ctx.set_min_disparity(dmin)
    ctx.set_mode(d2pc.MODE_PARITY)
    full, _, _, roi_n = run_batch(ctx, frames, want_index=False, scale=scale)
    ctx.set_mode(d2pc.MODE_COMPACT)
    st0 = ctx.compact_stats()
    pts, idx, counts, _ = run_batch(ctx, frames, want_index=want_index, scale=scale)
    st = ctx.compact_stats()
    assert st["timeouts"] == st0["timeouts"], what
    if algo in (2, 3):
        assert st["launches"] == st0["launches"] + 1 and st["twopass_fallbacks"] == st0["twopass_fallbacks"], (what, st0, st)
    else:
        assert st["launches"] == st0["launches"], (what, st0, st)
    assert not np.any(counts == 0xFFFFFFFF), what
    h, w = frames[0].shape
    b = ctx.config().border
    v, u = np.mgrid[b:h - b, b:w - b]
    pix = (v * w + u).reshape(-1).astype(np.uint32)
    for f in range(len(frames)):
        d = (decoded if decoded is not None else frames)[f][b:h - b, b:w - b].reshape(-1)
        fp = full[f, :roi_n]
        keep = np.isfinite(fp[:, :3]).all(axis=1) & ~(d <= np.float32(dmin))
        assert counts[f] == keep.sum(), f"{what} frame {f}: count {counts[f]} != {keep.sum()}"
        n = int(counts[f])
        assert np.array_equal(pts[f, :n].view(np.uint32), fp[keep].view(np.uint32)), f"{what} frame {f}: points"
        if want_index:
            assert np.array_equal(idx[f, :n], pix[keep]), f"{what} frame {f}: indices"
    return pts, idx, counts


from disparity_to_point_cloud_amd.synth import frame_seed, synth_disparity  # noqa: E402,F401
