"""The device medians and the tile-fused callback kernels (d2pc_callback.hip) on value distributions that reach the
whole byte range: two-level images whose window counts run through 0..k^2 at every bit plane, narrow bands at the
ends of the range, and piecewise-planar scenes whose k = 11 median takes all 256 byte values inside the ROI, so that
every entry of the per-byte tables (1/W, Z, validity class) is read.  Inputs: tests/value_patterns.py; each test also
asserts that its input reaches what it was built to reach."""
import functools

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import oracle
import value_patterns as vp
from helpers import assert_points_close

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

KS = [3, 5, 7, 9, 11]


def _stage(frames, pitch, seed=0):
    """Frames into one (n, h, pitch) device batch; the columns past the width hold junk the kernels must not read."""
    h, w = frames[0].shape
    buf = np.random.default_rng(seed).integers(0, 256, size=(len(frames), h, pitch)).astype(np.uint8)
    buf[:, :, :w] = np.stack(frames)
    return torch.from_numpy(buf).cuda()


def _assert_covers_every_byte(med, border, what):
    got = vp.roi_values(med, border)
    assert len(got) == 256, f"{what}: the ROI median misses {sorted(set(range(256)) - set(got.tolist()))[:8]}"


@functools.lru_cache(maxsize=None)
def _median_set(w, h, k):
    """All families at one shape: both two-level forms of every pair, the narrow bands, two smooth scenes."""
    frames = []
    for seed in (2, 3):   # each pair as a row ramp once and with per-tile densities once
        for i, (img, lo, hi) in enumerate(vp.two_level_frames(seed, h, w, k)):
            if (i + seed) % 2 == 0:   # the row ramp: every window count 0..k^2
                assert set(np.unique(vp.window_counts(img == hi, k)).tolist()) == set(range(k * k + 1)), (lo, hi)
            frames.append(img)
    frames += [vp.narrow_band(np.random.default_rng(i), h, w, lo, width) for i, (lo, width) in enumerate(vp.NARROW_BANDS)]
    frames += vp.smooth_frames(2, 2, h, w)
    return frames, [oracle.median_u8(f, k) for f in frames]


@pytest.mark.parametrize("w,h,pitch", [(752, 480, 752), (520, 261, 533), (257, 33, 270)])
@pytest.mark.parametrize("k", KS)
def test_median_device_on_value_patterns(k, w, h, pitch):
    """d2pc_median_device, every algorithm (1: per pixel, 2: bit-sliced, 0: the library's choice; 3: the lane-pair
    select of the experiment build), all families in one launch, strided source rows: byte-equal to the oracle;
    the destination's pad columns untouched."""
    frames, want = _median_set(w, h, k)
    if k == 11:
        _assert_covers_every_byte(want[-1], 7 if h < 128 else 40, "smooth scene")
    n = len(frames)
    src = _stage(frames, pitch)
    for variant, algo in ((None, 1), (None, 2), (None, 0), ("exp", 3)):
        dst = torch.full((n, h, pitch + 3), 77, dtype=torch.uint8, device="cuda")
        with d2pc.Context(q=d2pc.make_q(), variant=variant) as ctx:
            ctx.set_tuning("median_algo", algo)
            ctx.median_device(src.data_ptr(), w, h, pitch, pitch * h, n, dst.data_ptr(), pitch + 3, (pitch + 3) * h, k,
                              torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        got = dst.cpu().numpy()
        for f in range(n):
            assert np.array_equal(got[f, :, :w], want[f]), f"algo {algo}, frame {f}"
        assert (got[:, :, w:] == 77).all(), f"algo {algo}: wrote past the width"


@pytest.mark.parametrize("w,h,border", [(752, 480, 40), (520, 261, 40), (520, 261, 7), (257, 33, 7)])
def test_median_roi_device_on_value_patterns(w, h, border):
    """d2pc_median_roi_device on smooth scenes and two-level images: the whole-image median inside the ROI, the fill
    of 77 untouched outside it."""
    frames = vp.smooth_frames(3, 4, h, w) + [img for img, _, _ in vp.two_level_frames(3, h, w)]
    want = [oracle.median_u8(f, 11) for f in frames]
    for m in want[:4]:
        _assert_covers_every_byte(m, border, "smooth scene")
    n = len(frames)
    src = _stage(frames, w)
    inside = np.zeros((h, w), dtype=bool)
    inside[border:h - border, border:w - border] = True
    for algo in (1, 2):
        dst = torch.full_like(src, 77)
        with d2pc.Context(q=d2pc.make_q(), border=border) as ctx:
            ctx.set_tuning("median_algo", algo)
            ctx.median_roi_device(src.data_ptr(), w, h, w, w * h, n, dst.data_ptr(), w, w * h, 11,
                                  torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        got = dst.cpu().numpy()
        for f in range(n):
            assert np.array_equal(got[f][inside], want[f][inside]), f"algo {algo}, frame {f}"
            assert (got[f][~inside] == 77).all(), f"algo {algo}, frame {f}: wrote outside the ROI"


@functools.lru_cache(maxsize=None)
def _fused_set(w, h, border, k):
    """Four smooth scenes (two with holes and impulses) and one two-level image per pair; the ROI median of every
    scene takes all 256 byte values, that of every two-level image both of its values."""
    tl = vp.two_level_frames(1, h, w, k)
    frames = vp.smooth_frames(1, 4, h, w) + [img for img, _, _ in tl]
    med = [oracle.median_u8(f, k) for f in frames]
    for m in med[:4]:
        _assert_covers_every_byte(m, border, "smooth scene")
    for m, (_, lo, hi) in zip(med[4:], tl):
        assert {lo, hi} <= set(vp.roi_values(m, border).tolist()), (lo, hi)
    return frames, med


def _run_mono(ctx, b, src, dtype, w, h, row_stride, n, k, scale, key, fused):
    ctx.set_tuning(key, fused)
    b.points.fill_(0)
    b.index.fill_(-1)
    b.counts.fill_(-7)
    ctx.process_mono_device(src.data_ptr(), dtype, w, h, row_stride, row_stride * h, n, k, scale, b.points.data_ptr(),
                            b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check_async_error()
    return b.points.cpu().numpy().copy(), b.index.cpu().numpy().view(np.uint32).copy(), b.counts.cpu().numpy().view(np.uint32).copy()


FUSED_SHAPES = [(752, 480, 40, 765), (520, 261, 7, 520)]   # (w, h, border, source row stride)


@pytest.mark.parametrize("scale", [0.125, 1.0])
@pytest.mark.parametrize("general_q", [0, 1])
@pytest.mark.parametrize("k", [11, 9])
@pytest.mark.parametrize("w,h,border,pitch", FUSED_SHAPES)
def test_fused_parity_callback_on_value_patterns(w, h, border, pitch, k, general_q, scale):
    """k_callback_bs against the filter launch + reprojection launch (bitwise: points, indices, counts) and the oracle
    (<= 1 ulp in the default form, 0 ulp in a named one), in every reproject form."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    frames, med = _fused_set(w, h, border, k)
    n = len(frames)
    src = _stage(frames, pitch)
    with d2pc.Context(q=q, border=border) as ctx:
        ctx.set_test_hook("force_general_q", general_q)
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        for form in (d2pc.FORM_DEFAULT, d2pc.FORM_CV24, d2pc.FORM_CV4):
            ctx.set_reproject_form(form)
            res = {fused: _run_mono(ctx, b, src, d2pc.DTYPE_U8, w, h, pitch, n, k, scale, "callback_fused", fused)
                   for fused in (1, 0)}
            for a, c in zip(res[1], res[0]):
                assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"form {form}: one kernel differs from two launches"
            if form == d2pc.FORM_DEFAULT:
                oform, ulp = (oracle.FORM_CV4, 0) if general_q else (oracle.FORM_CV24, 1)
            else:
                oform, ulp = (oracle.FORM_CV24 if form == d2pc.FORM_CV24 else oracle.FORM_CV4), 0
            pts = res[1][0]
            for f in range(n):
                want = oracle.reproject(med[f], q, border=border, scale=scale, form=oform)
                assert res[1][2][f] == len(want)
                assert_points_close(pts[f][:len(want)], want, max_ulp=ulp, rel=1e-5, what=f"form {form}, frame {f}")


@pytest.mark.parametrize("general_q", [0, 1])
@pytest.mark.parametrize("dmin", [-np.inf, 0.0, 15.875, 16.0, 31.75])
@pytest.mark.parametrize("w,h,border,pitch,k", [(752, 480, 40, 765, 11), (520, 261, 7, 520, 9)])
def test_fused_compact_callback_on_value_patterns(w, h, border, pitch, k, dmin, general_q):
    """k_callback_bs_compact_pipe (2), k_callback_bs_compact (1) against the two launches (0), bitwise, and the oracle,
    with disparity floors whose class boundary falls among the bytes present (x 1/8: bytes 0, 127, 128, 254)."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    frames, med = _fused_set(w, h, border, k)
    n = len(frames)
    src = _stage(frames, pitch)
    with d2pc.Context(q=q, border=border, mode=d2pc.MODE_COMPACT, min_disparity=dmin) as ctx:
        ctx.set_test_hook("force_general_q", general_q)
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        ctx.compact_stats_reset()
        res = {fused: _run_mono(ctx, b, src, d2pc.DTYPE_U8, w, h, pitch, n, k, 0.125, "callback_fused_compact", fused)
               for fused in (2, 1, 0)}
        assert ctx.compact_stats()["timeouts"] == 0
    for fused in (2, 1):
        assert np.array_equal(res[fused][2], res[0][2]), f"counts differ (form {fused})"
        for a, c in zip(res[fused], res[0]):
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"form {fused} differs from the two launches"
    oform, ulp = (oracle.FORM_CV4, 0) if general_q else (oracle.FORM_CV24, 1)
    pts, idx, cnt = res[2]
    for f in range(n):
        want, wi = oracle.reproject_compact(med[f], q, border=border, scale=0.125, form=oform, min_disparity=dmin)
        assert cnt[f] == len(want), f"frame {f}"
        assert np.array_equal(idx[f][:len(wi)], wi), f"frame {f}"
        if len(want):
            assert_points_close(pts[f][:len(want)], want, max_ulp=ulp, rel=1e-5, what=f"frame {f}")


@pytest.mark.parametrize("fused", [1, 0])
@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
def test_mono16_smooth_scenes_through_the_whole_callback(mode, fused):
    """Smooth scenes as 16-bit frames (value x 257 + noise in +-128) through d2pc_process_mono_device: rescale,
    median 11, x 1/8, reproject -- against oracle.mono16_to_mono8 -> median -> reproject."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 4, 480, 752
    rng = np.random.default_rng(16)
    imgs = np.stack([np.clip(f.astype(np.int32) * 257 + rng.integers(-128, 129, size=(h, w)), 0, 65535).astype(np.uint16)
                     for f in vp.smooth_frames(0, n, h, w)])
    src = torch.from_numpy(imgs.view(np.int16)).cuda()
    with d2pc.Context(q=q, mode=mode) as ctx:
        ctx.set_tuning("median_algo", 2)
        ctx.set_tuning("callback_fused", fused)
        ctx.set_tuning("callback_fused_compact", 2 if fused else 0)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        pts, idx, cnt = _run_mono(ctx, b, src, d2pc.DTYPE_MONO16, w, h, 2 * w, n, 11, 0.125, "callback_fused", fused)
        if mode == d2pc.MODE_COMPACT:
            assert ctx.compact_stats()["timeouts"] == 0
    for f in range(n):
        filt = oracle.median_u8(oracle.mono16_to_mono8(imgs[f]), 11)
        _assert_covers_every_byte(filt, 40, f"frame {f}")
        if mode == d2pc.MODE_PARITY:
            want = oracle.reproject(filt, q, border=40, scale=0.125)
        else:
            want, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125)
            assert np.array_equal(idx[f][:len(wi)], wi), f"frame {f}"
        assert cnt[f] == len(want)
        assert_points_close(pts[f][:len(want)], want, max_ulp=1, rel=1e-5, what=f"frame {f}")


def _device_scenes(n, h, w, holes, seed):
    """n smooth scenes rendered on the device: value_patterns.scene_pieces' planes, +-2 noise and, with `holes`,
    ~30 % zero blocks of 32 x 32."""
    g = torch.Generator(device="cuda").manual_seed(seed)
    rng = np.random.default_rng(seed)
    out = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
    x = torch.arange(w, dtype=torch.float64, device="cuda")[None, :]
    y = torch.arange(h, dtype=torch.float64, device="cuda")[:, None]
    for f in range(n):
        gx, gy, c = (np.empty(w) for _ in range(3))
        for x0, x1, a, b_, c_ in vp.scene_pieces(rng, h, w):
            gx[x0:x1], gy[x0:x1], c[x0:x1] = a, b_, c_
        phase = torch.from_numpy(gx).cuda()[None, :] * x + torch.from_numpy(gy).cuda()[None, :] * y + torch.from_numpy(c).cuda()[None, :]
        t = 1.0 - (2.0 * (phase - phase.floor()) - 1.0).abs()
        v = ((t - 0.12) / 0.76).clamp(0.0, 1.0) * 255.0
        v += torch.randint(-2, 3, (h, w), device="cuda", generator=g, dtype=torch.int32)
        out[f] = v.round().clamp(0, 255).to(torch.uint8)
        del phase, t, v
    if holes:
        m = torch.rand((n, (h + 31) // 32, (w + 31) // 32), device="cuda", generator=g) < 0.3
        out[m.repeat_interleave(32, dim=1).repeat_interleave(32, dim=2)[:, :h, :w]] = 0
    return out


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
def test_callback_body_on_smooth_scenes_at_the_benchmark_size(mode):
    """16 x 3840x2160 smooth scenes (with zero holes in COMPACT): the one-kernel callback body against the two launches,
    compared on the device; two frames against the oracle (the fast median, pinned to the checker), their ROI median
    taking all 256 byte values."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 16, 2160, 3840
    compact = mode == d2pc.MODE_COMPACT
    src = _device_scenes(n, h, w, compact, 46 + mode)
    key, forms = ("callback_fused_compact", (2, 1, 0)) if compact else ("callback_fused", (1, 0))
    with d2pc.Context(q=q, mode=mode) as ctx:
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        s = torch.cuda.current_stream().cuda_stream
        keep = {}
        for fused in forms:
            ctx.set_tuning(key, fused)
            b.points.fill_(0)
            b.index.fill_(-1)
            b.counts.fill_(0)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), s)
            torch.cuda.synchronize()
            ctx.check_async_error()
            keep[fused] = (b.points.view(torch.int32).clone(), b.index.clone(), b.counts.clone())
        for fused in forms[:-1]:
            for x, y in zip(keep[fused], keep[0]):
                assert torch.equal(x, y), f"form {fused}"
        del keep
        res = b.results()
        if compact:
            assert ctx.compact_stats()["timeouts"] == 0
    imgs = src.cpu().numpy()
    for f in (0, 13):
        filt = oracle.median_u8_fast(imgs[f], 11)
        _assert_covers_every_byte(filt, 40, f"frame {f}")
        if compact:
            want, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125)
            assert np.array_equal(res[f][1], wi)
        else:
            want = oracle.reproject(filt, q, border=40, scale=0.125)
        assert len(res[f][0]) == len(want)
        assert_points_close(res[f][0], want, max_ulp=1, rel=1e-5, what=f"frame {f}")
