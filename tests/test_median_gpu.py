"""GPU tests of the device median (cv::medianBlur(...,11), cpp:55-57) and of
the fused callback body d2pc_process_mono8 (cpp:55-85) against the oracle."""
import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import oracle
from helpers import assert_points_close

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _median_gpu(ctx, imgs, k, algo=0):
    ctx.set_tuning("median_algo", algo)
    src = torch.from_numpy(np.stack(imgs)).cuda()
    n, h, w = src.shape
    dst = torch.full_like(src, 77)
    ctx.median_device(src.data_ptr(), w, h, w, w * h, n, dst.data_ptr(), w, w * h, k,
                      torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return dst.cpu().numpy()


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
@pytest.mark.parametrize("w,h", [(752, 480), (97, 131), (16, 64), (17, 65), (5, 3), (1, 1), (1, 40), (40, 1), (33, 7)])
def test_median_matches_oracle(k, w, h):
    rng = np.random.default_rng(w * 1000 + h + k)
    imgs = [rng.integers(0, 256, size=(h, w)).astype(np.uint8),
            (rng.integers(0, 4, size=(h, w)) * 85).astype(np.uint8)]  # many ties
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        got = _median_gpu(ctx, imgs, k)
    for g, img in zip(got, imgs):
        assert np.array_equal(g, oracle.median_u8(img, k))


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
@pytest.mark.parametrize("w,h", [(752, 480), (97, 131), (256, 32), (257, 33), (300, 70), (5, 3), (1, 1), (1, 40), (40, 1),
                                 (1037, 45)])
def test_bit_sliced_median_matches_oracle(k, w, h):
    """d2pc_median_bs.hip (32 pixels per thread, one bit each) forced onto sizes the library would give to the
    per-pixel kernel: tiles cut by the right and bottom edges, images smaller than the window, ties."""
    rng = np.random.default_rng(w * 1000 + h + k)
    imgs = [rng.integers(0, 256, size=(h, w)).astype(np.uint8),
            (rng.integers(0, 4, size=(h, w)) * 85).astype(np.uint8),
            np.tile(np.arange(w, dtype=np.uint8), (h, 1))]
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        got = _median_gpu(ctx, imgs, k, algo=2)
        again = _median_gpu(ctx, imgs, k, algo=1)
    for g, a, img in zip(got, again, imgs):
        want = oracle.median_u8(img, k)
        assert np.array_equal(g, want)
        assert np.array_equal(a, want)


@pytest.mark.parametrize("k", [3, 5, 7, 9, 11])
def test_lane_pair_select_experiment_matches_oracle(k):
    """EXPERIMENT BUILD (median_algo 3, round 4's verdict item 3c): the bit-sliced select with the candidate window split
    over a lane pair (select2 in lab/d2pc_median_bs2_tile.hpp: 66 instead of 121 candidate words per lane at 11 x 11, four waves
    per SIMD).  Same bytes as the oracle on tiles cut by every edge, ties, images smaller than the window."""
    rng = np.random.default_rng(3000 + k)
    for (w, h) in ((752, 480), (97, 131), (256, 32), (257, 33), (300, 70), (5, 3), (1, 1), (1, 40), (40, 1), (1037, 45)):
        imgs = [rng.integers(0, 256, size=(h, w)).astype(np.uint8),
                (rng.integers(0, 4, size=(h, w)) * 85).astype(np.uint8),
                np.tile(np.arange(w, dtype=np.uint8), (h, 1))]
        with d2pc.Context(q=d2pc.make_q(), variant="exp") as ctx:
            got = _median_gpu(ctx, imgs, k, algo=3)
        for g, img in zip(got, imgs):
            assert np.array_equal(g, oracle.median_u8(img, k)), (k, w, h)


@pytest.mark.parametrize("algo", [1, 2])
def test_median_algorithms_on_strided_rows_and_roi(algo):
    """Row strides larger than the width, source and destination strides different, ROI-only output."""
    rng = np.random.default_rng(77 + algo)
    n, h, w, sp, dp, border = 3, 150, 333, 352, 340, 21
    src = torch.from_numpy(rng.integers(0, 256, size=(n, h, sp)).astype(np.uint8)).cuda()
    dst = torch.full((n, h, dp), 77, dtype=torch.uint8, device="cuda")
    with d2pc.Context(q=d2pc.make_q(), border=border) as ctx:
        ctx.set_tuning("median_algo", algo)
        ctx.median_roi_device(src.data_ptr(), w, h, sp, sp * h, n, dst.data_ptr(), dp, dp * h, 11,
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got, imgs = dst.cpu().numpy(), src.cpu().numpy()[:, :, :w]
    inside = np.zeros((h, dp), dtype=bool)
    inside[border:h - border, border:w - border] = True
    for g, img in zip(got, imgs):
        want = oracle.median_u8(np.ascontiguousarray(img), 11)
        assert np.array_equal(g[:, :w][inside[:, :w]], want[inside[:, :w]])
        assert np.all(g[~inside] == 77), "pixels outside the ROI must not be written"


@pytest.mark.parametrize("k", [3, 11])
@pytest.mark.parametrize("w,h,border", [(752, 480, 40), (97, 131, 7), (100, 90, 40), (82, 81, 40), (64, 64, 0),
                                        (90, 200, 44), (3840, 2160, 40), (80, 80, 40), (30, 200, 20)])
def test_median_roi_only_equals_the_whole_image_filter_inside_the_roi(k, w, h, border):
    """The fused entry points filter only what cpp:70,72 read afterwards.  Inside the inset ROI every pixel must
    equal the whole-image median (windows still reach the true image edges); outside nothing is written."""
    rng = np.random.default_rng(w * 7 + h + k + border)
    imgs = [rng.integers(0, 256, size=(h, w)).astype(np.uint8) for _ in range(2)]
    src = torch.from_numpy(np.stack(imgs)).cuda()
    dst = torch.full_like(src, 77)
    with d2pc.Context(q=d2pc.make_q(), border=border) as ctx:
        ctx.median_roi_device(src.data_ptr(), w, h, w, w * h, 2, dst.data_ptr(), w, w * h, k,
                              torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    got = dst.cpu().numpy()
    inside = np.zeros((h, w), dtype=bool)
    if w > 2 * border and h > 2 * border:
        inside[border:h - border, border:w - border] = True
    for g, img in zip(got, imgs):
        want = oracle.median_u8(img, k)
        assert np.array_equal(g[inside], want[inside])
        assert np.all(g[~inside] == 77), "pixels outside the ROI must not be written"


def test_median_4k_batch_and_constant_images():
    rng = np.random.default_rng(2)
    a = rng.integers(0, 256, size=(2160, 3840)).astype(np.uint8)
    b = np.full((2160, 3840), 200, dtype=np.uint8)
    b[1000:1100, 2000:2100] = 0
    want = [oracle.median_u8(a, 11), oracle.median_u8(b, 11)]
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        for algo in (0, 1, 2):  # 0: the library's choice (bit-sliced at this size)
            got = _median_gpu(ctx, [a, b], 11, algo)
            assert np.array_equal(got[0], want[0]), algo
            assert np.array_equal(got[1], want[1]), algo


def test_median_rejects_bad_arguments():
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        x = torch.zeros((8, 8), dtype=torch.uint8, device="cuda")
        y = torch.zeros_like(x)
        for k in (0, 1, 2, 4, 13):
            with pytest.raises(d2pc.D2pcError) as e:
                ctx.median_device(x.data_ptr(), 8, 8, 8, 64, 1, y.data_ptr(), 8, 64, k)
            assert e.value.status == 1
        with pytest.raises(d2pc.D2pcError):
            ctx.median_device(x.data_ptr(), 8, 8, 8, 64, 1, x.data_ptr(), 8, 64, 3)  # in place
        with pytest.raises(d2pc.D2pcError):
            ctx.median_device(x.data_ptr(), 8, 8, 4, 64, 1, y.data_ptr(), 8, 64, 3)  # stride < width
        # the codes, and with two faults at once their order: pointers, ksize, sizes, row strides, frame strides
        lib, s, d = d2pc.load_library(), x.data_ptr(), y.data_ptr()
        for fn in (lib.d2pc_median_device, lib.d2pc_median_roi_device):
            for args, status in (((s, 8, 8, 4, 64, 1, s, 8, 64, 3), 1), ((s, 0, 8, 8, 64, 1, d, 8, 64, 4), 1),
                                 ((s, 0, 8, 4, 64, 1, d, 8, 64, 3), 3), ((s, 8, 8, 1 << 32, 64, 1, d, 8, 64, 3), 3),
                                 # two frames of 6 x 4 on a pitch of 8: a frame is its whole rows (4 * 8 bytes) here, not
                                 # the 3 * 8 + 6 bytes up to its last pixel
                                 ((s, 6, 4, 8, 30, 2, d, 8, 32, 3), 3), ((s, 6, 4, 8, 32, 2, d, 8, 31, 3), 3),
                                 ((s, 6, 4, 8, 32, 2, d, 8, 32, 3), 0)):
                assert fn(ctx._h, *args, None) == status, args
        torch.cuda.synchronize()


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
def test_process_mono8_is_the_callback_body(mode):
    """median 11 -> x1/8 -> reproject + pack, native 752x480 geometry."""
    rng = np.random.default_rng(9)
    img = rng.integers(0, 256, size=(480, 752)).astype(np.uint8)
    img[100:180, 300:420] = 0  # an invalid region that survives the median
    q = d2pc.make_q()
    med = oracle.median_u8(img, 11)
    with d2pc.Context(q=q, mode=mode) as ctx:
        got, idx = ctx.process_mono8(img, median_ksize=11, scale=0.125, want_index=True)
        raw, _ = ctx.process_mono8(img, median_ksize=0, scale=0.125, want_index=True)
    if mode == d2pc.MODE_PARITY:
        want = oracle.reproject(med, q, border=40, scale=0.125)
        assert len(got) == 268800
    else:
        want, wi = oracle.reproject_compact(med, q, border=40, scale=0.125)
        assert np.array_equal(idx, wi)
    assert_points_close(got, want, max_ulp=1, rel=1e-5, what="mono8 callback")
    # ksize 0 = no median
    want_raw = (oracle.reproject(img, q, border=40, scale=0.125) if mode == d2pc.MODE_PARITY
                else oracle.reproject_compact(img, q, border=40, scale=0.125)[0])
    assert_points_close(raw, want_raw, max_ulp=1)


# ---- cv_bridge mono16 -> mono8 on the device (cpp:50) -----------------------------
@pytest.mark.parametrize("w,h", [(640, 480), (752, 480), (1, 1), (3, 5), (5, 3), (129, 7), (1000, 3)])
def test_mono16_to_mono8_device_matches_oracle(w, h):
    rng = np.random.default_rng(w * 31 + h)
    imgs = np.stack([rng.integers(0, 65536, size=(h, w)).astype(np.uint16),
                     (rng.integers(0, 256, size=(h, w)) * 257).astype(np.uint16)])    # exact multiples: k*257 -> k
    imgs[0].flat[: min(imgs[0].size, 8)] = [0, 128, 129, 385, 65535, 65407, 65406, 32896][: min(imgs[0].size, 8)]  # .5 ties
    src = torch.from_numpy(imgs.view(np.int16)).cuda()
    dst = torch.full((2, h, w + 3), 7, dtype=torch.uint8, device="cuda")
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        ctx.mono16_to_mono8_device(src.data_ptr(), w, h, 2 * w, 2 * w * h, 2, dst.data_ptr(), w + 3, (w + 3) * h,
                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = dst.cpu().numpy()
        for f in range(2):
            assert np.array_equal(got[f, :, :w], oracle.mono16_to_mono8(imgs[f]))
            assert (got[f, :, w:] == 7).all()
        with pytest.raises(d2pc.D2pcError):
            ctx.mono16_to_mono8_device(src.data_ptr(), w, h, 2 * w - 1 if w > 1 else 1, 0, 1, dst.data_ptr(), w + 3, 0)
        with pytest.raises(d2pc.D2pcError):
            ctx.mono16_to_mono8_device(src.data_ptr(), w, h, 2 * w, 0, 1, src.data_ptr(), w, 0)


def test_mono16_to_mono8_device_refusal_codes_and_their_order():
    """Pointers, then sizes, then row strides / frame strides / alignment, then the overlap: one call each, none launches."""
    src = torch.zeros((2, 8, 8), dtype=torch.int16, device="cuda")
    dst = torch.full((2, 8, 8), 7, dtype=torch.uint8, device="cuda")
    s, d = src.data_ptr(), dst.data_ptr()
    with d2pc.Context(q=d2pc.make_q()) as ctx:
        call = d2pc.load_library().d2pc_mono16_to_mono8_device
        for args, status in (((None, 0, 8, 16, 128, 2, d, 8, 64), 1), ((s, 0, 8, 15, 128, 2, d, 8, 64), 3),
                             ((s, 8, 8, 15, 128, 2, s, 8, 64), 3), ((s, 8, 8, 14, 128, 2, d, 8, 64), 3),
                             ((s, 8, 8, 16, 127, 2, s, 8, 64), 3), ((s, 8, 8, 16, 129, 2, d, 8, 64), 3),
                             ((s, 8, 8, 16, 128, 2, d, 8, 63), 3), ((s + 1, 8, 8, 16, 128, 2, s, 8, 64), 3),
                             ((s, 8, 8, 1 << 32, 128, 1, d, 8, 64), 3), ((s, 8, 8, 16, 128, 2, s + 255, 8, 64), 1),
                             ((s, 8, 8, 16, 7, 1, d, 8, 7), 0)):  # one frame: the frame strides do not count
            assert call(ctx._h, *args, None) == status, args
        torch.cuda.synchronize()
    assert (dst[1] == 7).all() and (dst[0] == 0).all()  # only the last call ran, on one frame


def test_mono16_to_mono8_device_on_degenerate_shapes():
    """Both index forms of the rescale kernel (a grid of rows / one flat index per frame) at their limits: more rows
    than a grid dimension holds, rows of one pixel, rows that fill whole waves exactly."""
    rng = np.random.default_rng(16)
    for h, w in ((70000, 512), (70000, 9), (3, 1), (5, 4096), (1, 65535)):
        img = rng.integers(0, 65536, size=(h, w)).astype(np.uint16)
        src = torch.from_numpy(img.view(np.int16)).cuda()
        dst = torch.zeros((h, w), dtype=torch.uint8, device="cuda")
        with d2pc.Context(q=d2pc.make_q()) as ctx:
            ctx.mono16_to_mono8_device(src.data_ptr(), w, h, 2 * w, 2 * w * h, 1, dst.data_ptr(), w, w * h,
                                       torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
        assert np.array_equal(dst.cpu().numpy(), oracle.mono16_to_mono8(img)), (h, w)


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
@pytest.mark.parametrize("k", [0, 11])
def test_process_mono16_is_the_whole_callback(mode, k):
    """cpp:50-85 for a mono16 frame: rescale, median, x 1/8, reproject -- all on the device."""
    from helpers import synth_disparity
    q = d2pc.make_q()
    rng = np.random.default_rng(k + mode)
    for img in (synth_disparity(1, 0, 640, 480, "mono16"), rng.integers(0, 65536, size=(131, 203)).astype(np.uint16)):
        m8 = oracle.mono16_to_mono8(img)
        filt = oracle.median_u8(m8, k) if k else m8
        with d2pc.Context(q=q, mode=mode) as ctx:
            if mode == d2pc.MODE_PARITY:
                got = ctx.process_mono16(img, median_ksize=k)
                assert_points_close(got, oracle.reproject(filt, q, border=40, scale=0.125), max_ulp=1)
            else:
                gp, gi = ctx.process_mono16(img, median_ksize=k, want_index=True)
                wp, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125)
                assert np.array_equal(gi, wi)
                assert_points_close(gp, wp, max_ulp=1)
            with pytest.raises(d2pc.D2pcError):
                ctx.process_mono16(img, median_ksize=4)


def test_callback_body_is_graph_capturable():
    """mono16 rescale -> median 11 -> reproject, device-resident, captured into ONE hipGraph and replayed."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    rng = np.random.default_rng(8)
    imgs = rng.integers(0, 65536, size=(3, 240, 376)).astype(np.uint16)
    n, h, w = imgs.shape
    with d2pc.Context(q=q) as ctx:
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8)
        src = torch.from_numpy(imgs.view(np.int16)).cuda()
        m8 = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            def body():
                s = torch.cuda.current_stream().cuda_stream
                ctx.mono16_to_mono8_device(src.data_ptr(), w, h, 2 * w, 2 * w * h, n, m8.data_ptr(), w, w * h, s)
                ctx.median_device(m8.data_ptr(), w, h, w, w * h, n, b.disp.data_ptr(), w, w * h, 11, s)
                b.launch(scale=0.125)
            body()                      # warm-up outside the capture
            side.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=side):
                body()
            b.points.zero_()
            src.copy_(torch.from_numpy(np.roll(imgs, 1, axis=0).view(np.int16)).cuda())   # new input, same graph
            g.replay()
        torch.cuda.synchronize()
        res = b.results()
    for f in range(n):
        want = oracle.reproject(oracle.median_u8(oracle.mono16_to_mono8(np.roll(imgs, 1, axis=0)[f]), 11), q, border=40,
                                scale=0.125)
        assert_points_close(res[f][0], want, max_ulp=1, what=f"graph replay, frame {f}")


@pytest.mark.parametrize("fused", [0, 1])
def test_process_mono_device_compact_warm_up_then_capture_on_the_same_stream(fused):
    """d2pc_process_mono_device in COMPACT mode, warmed up and then captured on ONE stream without d2pc_reserve_mono: the
    two-launch form's scratch (filtered + rescaled frames) and the compaction state are the stream's own eager buffers
    and the capture must take them over (advisor, round 4: both pools answered OUT_OF_MEMORY)."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    rng = np.random.default_rng(77)
    n, h, w = 3, 300, 900
    imgs = rng.integers(0, 65536, size=(n, h, w)).astype(np.uint16)
    imgs[rng.random(imgs.shape) < 0.3] = 0
    with d2pc.Context(q=q, mode=d2pc.MODE_COMPACT) as ctx:
        ctx.set_tuning("callback_fused_compact", 2 if fused else 0)
        ctx.set_tuning("callback_fused", fused)
        if fused:
            ctx.set_tuning("median_algo", 2)   # the tile-fused kernel serves launches the bit-sliced filter takes
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True, reserve=False)
        src = torch.from_numpy(imgs.view(np.int16)).cuda()
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())

        def body():
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_MONO16, w, h, 2 * w, 2 * w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), s.cuda_stream)
        with torch.cuda.stream(s):
            body()
            body()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                body()
        b.points.fill_(0)
        b.counts.fill_(0)
        torch.cuda.synchronize()
        g.replay()
        res = b.results()
        ctx.check_async_error()
    for f in range(n):
        wp, wi = oracle.reproject_compact(oracle.median_u8(oracle.mono16_to_mono8(imgs[f]), 11), q, border=40, scale=0.125)
        assert np.array_equal(res[f][1], wi), f"frame {f}"
        assert_points_close(res[f][0], wp, max_ulp=1, what=f"frame {f}")


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
@pytest.mark.parametrize("dtype", ["u8", "mono16"])
@pytest.mark.parametrize("chunks", [2, 0, 4])
def test_process_mono_device_is_the_callback_body_for_a_batch(mode, dtype, chunks):
    """d2pc_process_mono_device: (rescale ->) median 11 over the ROI -> x 1/8 -> reproject for a device-resident
    batch.  The product serves it in order on the caller's stream (`callback_chunks` 0 / 1, the only values it takes);
    the EXPERIMENT BUILD cuts it into `callback_chunks` chunks pipelined over two internal streams
    (lab/d2pc_capi_mono_overlap.hip).  The split must never show in the result."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    rng = np.random.default_rng(mode * 10 + chunks)
    n, h, w = 7, 2000, 2448   # 34 Mpixel: big enough for the overlapped path to be taken
    if dtype == "u8":
        imgs = rng.integers(0, 256, size=(n, h, w)).astype(np.uint8)
        src = torch.from_numpy(imgs).cuda()
        m8, dt, rs = imgs, d2pc.DTYPE_U8, w
    else:
        imgs = rng.integers(0, 65536, size=(n, h, w)).astype(np.uint16)
        src = torch.from_numpy(imgs.view(np.int16)).cuda()
        m8, dt, rs = np.stack([oracle.mono16_to_mono8(i) for i in imgs]), d2pc.DTYPE_MONO16, 2 * w
    with d2pc.Context(q=q, mode=mode, variant="exp" if chunks > 1 else None) as ctx:
        if chunks <= 1:   # the product library: nothing to cut the batch with
            with pytest.raises(d2pc.D2pcError) as e:
                ctx.set_tuning("callback_chunks", 2)
            assert e.value.status == 1   # D2PC_ERR_INVALID_ARG
            ctx.set_tuning("callback_chunks", 1)
        ctx.set_tuning("callback_chunks", chunks)           # 7 frames: chunks of 4+3 / 2+2+2+1
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        for _ in range(3):  # relaunch: streams, events and scratch are reused
            with torch.cuda.stream(side):
                b.points.fill_(0)   # on the caller's stream: the call must order itself behind it
                ctx.process_mono_device(src.data_ptr(), dt, w, h, rs, rs * h, n, 11, 0.125, b.points.data_ptr(),
                                        b.index.data_ptr(), b.stride, b.counts.data_ptr(), side.cuda_stream)
            side.synchronize()   # the caller's stream alone: the internal streams must have joined it
        res = b.results()
        ctx.check_async_error()
    for f in range(n):
        filt = oracle.median_u8(m8[f], 11)
        pts, idx = res[f]
        if mode == d2pc.MODE_PARITY:
            want = oracle.reproject(filt, q, border=40, scale=0.125)
            assert len(pts) == len(want)
        else:
            want, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125)
            assert np.array_equal(idx, wi)
        assert_points_close(pts, want, max_ulp=1, rel=1e-5, what=f"frame {f}")


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
@pytest.mark.parametrize("dtype", ["u8", "mono16"])
@pytest.mark.parametrize("k", [3, 11])
def test_the_three_doors_of_the_callback_body_give_the_same_cloud(mode, dtype, k):
    """One frame through the three entry points that run (rescale ->) median(ROI) -> reproject: d2pc_process_mono8 / 16
    (pageable numpy), the pipelined host path (staged and direct_host_write) and d2pc_process_mono_device with one frame.
    Each keeps its own pitches -- the synchronous path packs to 256 bytes, the pipeline keeps the caller's stride for
    8-bit frames, the device path reads the caller's layout and packs its scratch -- so the shape is one at which a
    mix-up shows: 333 samples a row (no multiple of 256 bytes), caller rows padded by 13 samples that hold the largest
    value (read as pixels they would change the median), border 5 < the window's reach.  Every door equals the oracle
    (indices exact, points within 1 ulp) and the doors equal each other bit for bit."""
    from textured_expect import roi_pixels
    q = d2pc.make_q()
    w, h, border, pad = 333, 70, 5, 13
    u8 = dtype == "u8"
    np_dt, top = (np.uint8, 255) if u8 else (np.uint16, 65535)
    rng = np.random.default_rng(4 * k + 2 * mode + u8)
    wide = np.full((h, w + pad), top, dtype=np_dt)
    wide[:, :w] = rng.integers(0, top + 1, size=(h, w))
    wide[:, :w][rng.random((h, w)) < 0.3] = 0
    wide[20:45, 100:200] = 0                      # holes that survive the filter: COMPACT drops points
    img = wide[:, :w]                             # the caller's rows: w + 13 samples apart
    m8 = np.ascontiguousarray(img) if u8 else oracle.mono16_to_mono8(np.ascontiguousarray(img))
    filt = oracle.median_u8(m8, k)
    if mode == d2pc.MODE_PARITY:
        want_p, want_i = oracle.reproject(filt, q, border=border, scale=0.125), roi_pixels(h, w, border)
    else:
        want_p, want_i = oracle.reproject_compact(filt, q, border=border, scale=0.125)
        assert 0 < len(want_i) < (w - 2 * border) * (h - 2 * border)
    roi_n = (w - 2 * border) * (h - 2 * border)
    doors = {}
    with d2pc.Context(q=q, border=border, mode=mode) as ctx:
        doors["synchronous"] = (ctx.process_mono8 if u8 else ctx.process_mono16)(img, k, 0.125, want_index=True)
        for direct in (False, True):
            ctx.pipeline_configure(depth=1, direct_host_write=direct)
            ctx.pipeline_submit(np.ascontiguousarray(img), scale=0.125, median_ksize=k, want_index=True, mono16=not u8)
            doors["pipeline, direct" if direct else "pipeline, staged"] = ctx.pipeline_collect()[:2]
        src = torch.from_numpy(wide if u8 else wide.view(np.int16)).cuda()
        pts = torch.zeros((roi_n, 4), dtype=torch.float32, device="cuda")
        idx = torch.full((roi_n,), -1, dtype=torch.int32, device="cuda")
        cnt = torch.zeros(1, dtype=torch.int32, device="cuda")
        rs = wide.strides[0]
        ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8 if u8 else d2pc.DTYPE_MONO16, w, h, rs, rs * h, 1, k, 0.125,
                                pts.data_ptr(), idx.data_ptr(), roi_n, cnt.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ctx.check_async_error()
        n = roi_n if mode == d2pc.MODE_PARITY else int(cnt.item())
        doors["device"] = (pts.cpu().numpy()[:n], idx.cpu().numpy().view(np.uint32)[:n])
    for name, (p, i) in doors.items():
        assert np.array_equal(i, want_i), name
        assert_points_close(p, want_p, max_ulp=1, what=name)
    first_p = doors["synchronous"][0]      # (the indices are equal already: each equals the oracle's)
    for name, (p, _) in doors.items():
        assert np.array_equal(p.view(np.uint32), first_p.view(np.uint32)), f"{name} differs from the synchronous door"


def test_process_mono_device_rejects_bad_arguments_and_runs_in_order_under_capture():
    q = d2pc.make_q()
    rng = np.random.default_rng(5)
    imgs = rng.integers(0, 256, size=(4, 200, 320)).astype(np.uint8)
    n, h, w = imgs.shape
    src = torch.from_numpy(imgs).cuda()
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    with d2pc.Context(q=q) as ctx:
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8)
        args = (w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(), None, b.stride, b.counts.data_ptr())
        with pytest.raises(d2pc.D2pcError):
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_F32, *args)
        with pytest.raises(d2pc.D2pcError):
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 4, 0.125, b.points.data_ptr(), None,
                                    b.stride, b.counts.data_ptr())
        s = torch.cuda.current_stream().cuda_stream
        ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, *args, s)   # allocates the scratch
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):   # CU masks are a stream property a graph does not keep: in order on the capture stream
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, *args, torch.cuda.current_stream().cuda_stream)
        b.points.fill_(0)
        g.replay()
        res = b.results()
    for f in range(n):
        want = oracle.reproject(oracle.median_u8(imgs[f], 11), q, border=40, scale=0.125)
        assert_points_close(res[f][0], want, max_ulp=1, what=f"captured frame {f}")


@pytest.mark.parametrize("general_q", [0, 1])
@pytest.mark.parametrize("k,shape,border,scale", [(11, (3, 480, 752), 40, 0.125), (11, (2, 131, 203), 7, 0.37),
                                                  (9, (2, 300, 408), 40, 0.125), (11, (1, 97, 600), 0, 1.0),
                                                  (11, (2, 1080, 1920), 40, 0.125), (3, (2, 200, 520), 3, 0.125),
                                                  (5, (1, 131, 203), 0, 0.5), (7, (2, 90, 300), 11, 0.125)])
def test_tile_fused_callback_kernel_matches_the_two_launches_and_the_oracle(general_q, k, shape, border, scale):
    """k_callback_bs: the bit-sliced median of a 256 x 32 tile and, from the filtered bytes still in LDS, the tile's
    points (for stereoRectify's Q through a per-block table of 1/W and Z over the 256 byte values).  Forced onto
    small and ragged sizes (median_algo 2); must equal the filter launch + reprojection launch bit for bit --
    points, indices and counts -- and the oracle, for both forms of Q."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = shape
    rng = np.random.default_rng(n * h + w + k)
    pitch = w + 13
    imgs = rng.integers(0, 256, size=(n, h, pitch)).astype(np.uint8)
    src = torch.from_numpy(imgs).cuda()
    res = {}
    with d2pc.Context(q=q, border=border) as ctx:
        ctx.set_test_hook("force_general_q", general_q)
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        s = torch.cuda.current_stream().cuda_stream
        for fused in (1, 0):
            ctx.set_tuning("callback_fused", fused)
            for _ in range(2):
                b.points.fill_(0)
                b.index.fill_(-1)
                b.counts.fill_(0)
                ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, pitch, pitch * h, n, k, scale,
                                        b.points.data_ptr(), b.index.data_ptr(), b.stride, b.counts.data_ptr(), s)
            torch.cuda.synchronize()
            res[fused] = (b.points.cpu().numpy().copy(), b.index.cpu().numpy().copy(), b.counts.cpu().numpy().copy())
        ctx.check_async_error()
    for a, c in zip(res[1], res[0]):
        assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), "tile-fused kernel differs from the two launches"
    pts = res[1][0].reshape(n, -1, 4)
    form, ulp = (oracle.FORM_CV4, 0) if general_q else (oracle.FORM_CV24, 1)  # the general kernel IS OpenCV 4's association
    for f in range(n):
        want = oracle.reproject(oracle.median_u8(np.ascontiguousarray(imgs[f, :, :w]), k), q, border=border, scale=scale, form=form)
        assert res[1][2].view(np.uint32)[f] == len(want)
        assert_points_close(pts[f][:len(want)], want, max_ulp=ulp, rel=1e-5, what=f"frame {f}")


@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
@pytest.mark.parametrize("form,oform", [(24, oracle.FORM_CV24), (4, oracle.FORM_CV4)])
def test_callback_body_in_one_opencv_generation_bit_for_bit(mode, form, oform, general):
    """cpp:55-85 as a node linked against OpenCV 2.4 (form 24) or 3/4 (form 4) computes it: median, x 1/8, that
    generation's reprojectImageTo3D arithmetic, ROI pack -- 0 ulp, one kernel and two launches."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 2, 480, 752
    imgs = np.random.default_rng(form).integers(0, 256, size=(n, h, w)).astype(np.uint8)
    imgs[1, 100:300, 200:500] = 0
    src = torch.from_numpy(imgs).cuda()
    key = "callback_fused" if mode == d2pc.MODE_PARITY else "callback_fused_compact"
    with d2pc.Context(q=q, border=40, mode=mode) as ctx:
        ctx.set_reproject_form(form)
        ctx.set_test_hook("force_general_q", general)   # 0: the specialised kinds (tables of 1/W per byte value), 1: the general kernel
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        for fused in ((2, 1, 0) if mode == d2pc.MODE_COMPACT else (1, 0)):
            ctx.set_tuning(key, fused)
            b.points.fill_(0); b.index.fill_(-1); b.counts.fill_(0)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            pts, idx, cnt = b.points.cpu().numpy().reshape(n, -1, 4), b.index.cpu().numpy().view(np.uint32), b.counts.cpu().numpy()
            for f in range(n):
                filt = oracle.median_u8(imgs[f], 11)
                if mode == d2pc.MODE_COMPACT:
                    want, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125, form=oform)
                    assert np.array_equal(idx[f][:len(wi)], wi)
                else:
                    want = oracle.reproject(filt, q, border=40, scale=0.125, form=oform)
                assert cnt[f] == len(want)
                got = pts[f][:len(want)]
                nan = np.isnan(want)
                assert np.array_equal(nan, np.isnan(got))
                assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), f"fused={fused} frame {f}"
        ctx.check_async_error()


@pytest.mark.parametrize("scale", [float("inf"), float("nan"), -0.125, 3.0e38, 0.0, 1e-45])
def test_tile_fused_callback_kernel_with_degenerate_scales(scale):
    """The table of 1/W over the byte values must reproduce reproject()'s inf / NaN / signed-zero behaviour: byte 0
    times inf is NaN, W = 0 gives infinities, FLT_MAX hits the bigZ rule ...  Bitwise against the two launches."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    n, h, w = 2, 90, 300
    imgs = np.random.default_rng(3).integers(0, 256, size=(n, h, w)).astype(np.uint8)
    imgs[0, :, :150] = 0
    src = torch.from_numpy(imgs).cuda()
    res = {}
    with d2pc.Context(q=d2pc.make_q(), border=7) as ctx:
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8)
        for fused in (1, 0):
            ctx.set_tuning("callback_fused", fused)
            b.points.fill_(0)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, scale, b.points.data_ptr(), None,
                                    b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            res[fused] = b.points.cpu().numpy().view(np.uint32).copy()
    assert np.array_equal(res[1], res[0])


def test_tile_fused_callback_kernel_is_capturable_without_a_warm_up_call():
    """The one-kernel form needs no scratch for filtered frames, so the very first call of a size may already be
    inside a stream capture; the graph replays onto wiped outputs."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 3, 200, 520
    imgs = np.random.default_rng(8).integers(0, 256, size=(n, h, w)).astype(np.uint8)
    src = torch.from_numpy(imgs).cuda()
    with d2pc.Context(q=q) as ctx:
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(), None,
                                    b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        for _ in range(2):
            b.points.fill_(0)
            b.counts.fill_(0)
            g.replay()
            res = b.results()
            for f in range(n):
                want = oracle.reproject(oracle.median_u8(imgs[f], 11), q, border=40, scale=0.125)
                assert_points_close(res[f][0], want, max_ulp=1, what=f"replayed frame {f}")


def test_callback_body_at_the_benchmark_size_one_kernel_equals_two_launches():
    """Config 4's geometry (16 x 3840x2160, 8-bit): the one-kernel callback body against the filter launch + reprojection
    launch, compared on the device; three frames of it against the oracle."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 16, 2160, 3840
    g = torch.Generator(device="cuda").manual_seed(44)
    src = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    with d2pc.Context(q=q) as ctx:
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        s = torch.cuda.current_stream().cuda_stream
        keep = {}
        for fused in (1, 0):
            ctx.set_tuning("callback_fused", fused)
            b.points.fill_(0)
            b.index.fill_(-1)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), s)
            torch.cuda.synchronize()
            keep[fused] = (b.points.view(torch.int32).clone(), b.index.clone(), b.counts.clone())
        for x, y in zip(keep[1], keep[0]):
            assert torch.equal(x, y)
        res = b.results()
    for f in (0, 7, 15):
        want = oracle.reproject(oracle.median_u8(src[f].cpu().numpy(), 11), q, border=40, scale=0.125)
        assert_points_close(res[f][0], want, max_ulp=1, rel=1e-5, what=f"frame {f}")


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
@pytest.mark.parametrize("dtype", ["u8", "mono16"])
def test_process_mono_device_two_launch_form_on_two_streams_in_flight(mode, dtype):
    """Advisor, round 2: the two-launch form of d2pc_process_mono_device kept its filtered / rescaled frames in ONE
    context-wide scratch, so two calls in flight on different streams overwrote each other's frames.  Two different
    batches, two streams, no synchronisation in between, many rounds: each must come out as its own."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    rng = np.random.default_rng(90 + mode)
    n, h, w = 5, 480, 752
    sets = []
    for _ in range(2):
        if dtype == "u8":
            imgs = rng.integers(0, 256, size=(n, h, w)).astype(np.uint8)
            sets.append((imgs, torch.from_numpy(imgs).cuda(), imgs))
        else:
            imgs = rng.integers(0, 65536, size=(n, h, w)).astype(np.uint16)
            sets.append((imgs, torch.from_numpy(imgs.view(np.int16)).cuda(), np.stack([oracle.mono16_to_mono8(i) for i in imgs])))
    dt, rs = (d2pc.DTYPE_U8, w) if dtype == "u8" else (d2pc.DTYPE_MONO16, 2 * w)
    with d2pc.Context(q=q, mode=mode) as ctx:
        ctx.set_tuning("callback_fused", 0)   # the filter launch + the reprojection launch: the form with scratch
        bs = [DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True) for _ in range(2)]
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for _ in range(10):
            for (_, src, _), b, s in zip(sets, bs, streams):
                ctx.process_mono_device(src.data_ptr(), dt, w, h, rs, rs * h, n, 11, 0.125, b.points.data_ptr(),
                                        b.index.data_ptr(), b.stride, b.counts.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        ctx.check_async_error()
        res = [b.results() for b in bs]
    for (_, _, m8), r in zip(sets, res):
        for f in range(n):
            filt = oracle.median_u8(m8[f], 11)
            pts, idx = r[f]
            if mode == d2pc.MODE_PARITY:
                want = oracle.reproject(filt, q, border=40, scale=0.125)
            else:
                want, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125)
                assert np.array_equal(idx, wi)
            assert_points_close(pts, want, max_ulp=1, rel=1e-5, what=f"frame {f}")


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
def test_process_mono_device_is_capturable_after_reserve_mono(mode):
    """d2pc_reserve_mono: the two-launch form (here: MONO16 + COMPACT-or-PARITY with callback_fused = 0) captured
    WITHOUT a warm-up call of that size; without the reservation the capture is refused cleanly."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    rng = np.random.default_rng(12)
    imgs = rng.integers(0, 65536, size=(3, 300, 412)).astype(np.uint16)
    n, h, w = imgs.shape
    src = torch.from_numpy(imgs.view(np.int16)).cuda()
    with d2pc.Context(q=q, mode=mode) as ctx:
        ctx.set_tuning("callback_fused", 0)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)

        def call():
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_MONO16, w, h, 2 * w, 2 * w * h, n, 11, 0.125,
                                    b.points.data_ptr(), b.index.data_ptr(), b.stride, b.counts.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        err = None
        with torch.cuda.graph(g):
            try:
                call()
            except d2pc.D2pcError as e:
                err = e
        assert err is not None and "reserve" in str(err)
        ctx.reserve_mono(d2pc.DTYPE_MONO16, w, h, n)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            call()
        for _ in range(2):
            b.points.fill_(0)
            b.counts.fill_(0)
            g.replay()
        res = b.results()
        ctx.check_async_error()
    for f in range(n):
        filt = oracle.median_u8(oracle.mono16_to_mono8(imgs[f]), 11)
        if mode == d2pc.MODE_PARITY:
            want = oracle.reproject(filt, q, border=40, scale=0.125)
        else:
            want, wi = oracle.reproject_compact(filt, q, border=40, scale=0.125)
            assert np.array_equal(res[f][1], wi)
        assert_points_close(res[f][0], want, max_ulp=1, what=f"captured frame {f}")


def _holey_images(rng, n, h, pitch, kind):
    imgs = rng.integers(0, 256, size=(n, h, pitch)).astype(np.uint8)
    if kind == "iid":       # ~half of the pixels zero: the median comes out zero in patches
        imgs[rng.random(imgs.shape) < 0.5] = 0
    elif kind == "blocky":  # whole regions without a match
        m = rng.random((n, (h + 31) // 32, (pitch + 31) // 32)) < 0.4
        imgs[np.repeat(np.repeat(m, 32, axis=1), 32, axis=2)[:, :h, :pitch]] = 0
    elif kind == "empty":
        imgs[:] = 0
    return imgs


@pytest.mark.parametrize("general_q", [0, 1])
@pytest.mark.parametrize("k,shape,border,scale,kind", [
    (11, (3, 480, 752), 40, 0.125, "iid"), (11, (2, 131, 203), 7, 0.37, "blocky"), (9, (2, 300, 408), 40, 0.125, "iid"),
    (11, (1, 97, 600), 0, 1.0, "blocky"), (11, (2, 1080, 1920), 40, 0.125, "blocky"), (3, (2, 200, 520), 3, 0.125, "iid"),
    (5, (1, 131, 203), 0, 0.5, "dense"), (7, (2, 90, 300), 11, 0.125, "empty"), (11, (5, 240, 1400), 16, 0.125, "iid")])
def test_tile_fused_compact_kernel_matches_the_two_launches_and_the_oracle(general_q, k, shape, border, scale, kind):
    """k_callback_bs_compact: median of a tile, then the tile's SURVIVING points in the CPU loop's row-major order,
    handed over between the tiles of a band inside one launch.  Points, indices and counts must equal the two-launch
    COMPACT path (filter launch + compaction launch) bit for bit, and the oracle; relaunched (state re-initialised)."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = shape
    rng = np.random.default_rng(n * h + w + k)
    pitch = w + 13
    imgs = _holey_images(rng, n, h, pitch, kind)
    src = torch.from_numpy(imgs).cuda()
    res = {}
    with d2pc.Context(q=q, border=border, mode=d2pc.MODE_COMPACT) as ctx:
        ctx.set_test_hook("force_general_q", general_q)
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        s = torch.cuda.current_stream().cuda_stream
        for fused in (2, 1, 0):   # pipelined persistent form, one tile per block, two launches
            ctx.set_tuning("callback_fused_compact", fused)
            for _ in range(3):
                b.points.fill_(0)
                b.index.fill_(-1)
                b.counts.fill_(-7)
                ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, pitch, pitch * h, n, k, scale,
                                        b.points.data_ptr(), b.index.data_ptr(), b.stride, b.counts.data_ptr(), s)
            torch.cuda.synchronize()
            ctx.check_async_error()
            res[fused] = (b.points.cpu().numpy().copy(), b.index.cpu().numpy().copy(), b.counts.cpu().numpy().copy())
        st = ctx.compact_stats()
        assert st["timeouts"] == 0
    for fused in (1, 2):
        assert np.array_equal(res[fused][2], res[0][2]), f"counts differ (form {fused})"
        for a, c in zip(res[fused], res[0]):
            assert np.array_equal(a.view(np.uint32), c.view(np.uint32)), f"tile-fused COMPACT kernel (form {fused}) differs from the two launches"
    pts, idx = res[1][0].reshape(n, -1, 4), res[1][1].view(np.uint32)
    form, ulp = (oracle.FORM_CV4, 0) if general_q else (oracle.FORM_CV24, 1)
    for f in range(n):
        want, wi = oracle.reproject_compact(oracle.median_u8(np.ascontiguousarray(imgs[f, :, :w]), k), q, border=border, scale=scale,
                                            form=form)
        assert res[1][2].view(np.uint32)[f] == len(want)
        assert np.array_equal(idx[f][:len(wi)], wi)
        if len(want):
            assert_points_close(pts[f][:len(want)], want, max_ulp=ulp, rel=1e-5, what=f"frame {f}")


@pytest.mark.parametrize("scale,dmin", [(float("inf"), -np.inf), (float("nan"), -np.inf), (-0.125, -np.inf), (3.0e38, -np.inf),
                                        (0.0, -np.inf), (1e-45, -np.inf), (0.125, 12.0), (0.125, 31.875), (1.3e-41, -np.inf)])
def test_tile_fused_compact_kernel_with_degenerate_scales_and_a_disparity_floor(scale, dmin):
    """The per-byte-value validity classes must reproduce point_is_valid(): infinities, NaNs, tiny W (the exact path),
    d <= min_disparity.  Bitwise against the two launches."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    n, h, w = 2, 90, 300
    imgs = np.random.default_rng(3).integers(0, 256, size=(n, h, w)).astype(np.uint8)
    imgs[0, :, :150] = 0
    src = torch.from_numpy(imgs).cuda()
    res = {}
    with d2pc.Context(q=d2pc.make_q(), border=7, mode=d2pc.MODE_COMPACT, min_disparity=dmin) as ctx:
        ctx.set_tuning("median_algo", 2)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        for fused in (2, 1, 0):
            ctx.set_tuning("callback_fused_compact", fused)
            b.points.fill_(0)
            b.index.fill_(-1)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, scale, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ctx.check_async_error()
            res[fused] = (b.points.cpu().numpy().view(np.uint32).copy(), b.index.cpu().numpy().copy(), b.counts.cpu().numpy().copy())
    for fused in (1, 2):
        for a, c in zip(res[fused], res[0]):
            assert np.array_equal(a, c), f"form {fused}"


@pytest.mark.parametrize("n,h,w", [(500, 120, 400), (1000, 120, 160)])
def test_tile_fused_compact_kernel_with_more_frames_than_resident_bands(n, h, w):
    """Advisor, round 3: a frame needs a whole band of its tiles (tiles_x blocks) resident at once, and blocks go round-robin
    over the launch's frames -- from ~resident / tiles_x frames on, no frame could finish band 0 and every wave spun out its
    wait budget.  400x120 (ROI 320x40: 2 tiles per band) x 500 frames is past that point on 256 CUs x 3 blocks; the host
    now cuts such calls into sub-batches.  Both forms of the kernel against the two launches, bitwise; no timeouts."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    rng = np.random.default_rng(n)
    imgs = rng.integers(0, 256, size=(n, h, w)).astype(np.uint8)
    imgs[rng.random((n, h, w)) < 0.3] = 0
    src = torch.from_numpy(imgs).cuda()
    res = {}
    with d2pc.Context(q=d2pc.make_q(), mode=d2pc.MODE_COMPACT) as ctx:
        ctx.set_tuning("median_algo", 2)
        ctx.set_tuning("spin_timeout_ms", 500)   # (a regression would otherwise spin 4 s per wave before failing)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        ctx.compact_stats_reset()
        for fused in (2, 1, 0):
            ctx.set_tuning("callback_fused_compact", fused)
            b.points.fill_(0)
            b.index.fill_(-1)
            b.counts.fill_(-7)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ctx.check_async_error()
            res[fused] = (b.points.cpu().numpy().view(np.uint32).copy(), b.index.cpu().numpy().copy(), b.counts.cpu().numpy().copy())
            assert not (res[fused][2].view(np.uint32) == 0xFFFFFFFF).any(), f"form {fused}: a frame reports a timed-out hand-off"
        assert ctx.compact_stats()["timeouts"] == 0
    for fused in (1, 2):
        for a, c in zip(res[fused], res[0]):
            assert np.array_equal(a, c), f"form {fused} differs from the two launches"
    for f in (0, n // 2, n - 1):
        want, wi = oracle.reproject_compact(oracle.median_u8(imgs[f], 11), d2pc.make_q(), border=40, scale=0.125)
        assert res[2][2].view(np.uint32)[f] == len(want)
        assert np.array_equal(res[2][1].view(np.uint32).reshape(n, -1)[f][:len(wi)], wi)


@pytest.mark.parametrize("n,h,w", [(2, 150, 4500), (2, 4300, 400), (3, 200, 4176)])
def test_tile_fused_compact_kernel_beyond_the_early_look_of_its_placing_words(n, h, w):
    """The pipelined kernel requests the words that place a tile early, into registers sized for images up to 16 tiles across
    (4,096 output columns) and 128 bands (4,096 output rows); beyond either it polls as before.  4500 wide = 18 tiles
    across, 4300 high = 132 bands, 4176 wide = exactly 16 tiles: all three against the two launches, bitwise, and the oracle.

    What this reaches: the three shapes have 54, 264 and 64 tiles per frame against resident / n = 384 or 256 blocks per
    frame on a 256-CU device, so the router gives every tile a block of its own.  A block then has no tile in waiting while
    it filters one: CbEarlyPlace::request and take never run, and every tile is placed by cb_look.  The test holds the
    one-tile-per-block routing of these sizes to the two launches; the early look itself, either side of its limits and in
    blocks that do walk tiles, is tests/test_callback_compact_occupancy_gpu.py's (`sixteen`, `seventeen`, `tall`)."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    rng = np.random.default_rng(h + w)
    imgs = rng.integers(0, 256, size=(n, h, w)).astype(np.uint8)
    imgs[rng.random((n, h, w)) < 0.3] = 0
    src = torch.from_numpy(imgs).cuda()
    res = {}
    with d2pc.Context(q=d2pc.make_q(), mode=d2pc.MODE_COMPACT) as ctx:
        ctx.set_tuning("median_algo", 2)
        ctx.set_tuning("spin_timeout_ms", 500)
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        for fused in (2, 0):
            ctx.set_tuning("callback_fused_compact", fused)
            b.points.fill_(0)
            b.index.fill_(-1)
            b.counts.fill_(-7)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            ctx.check_async_error()
            res[fused] = (b.points.cpu().numpy().view(np.uint32).copy(), b.index.cpu().numpy().copy(), b.counts.cpu().numpy().copy())
        assert ctx.compact_stats()["timeouts"] == 0
    for a, c in zip(res[2], res[0]):
        assert np.array_equal(a, c), "the pipelined kernel differs from the two launches"
    want, wi = oracle.reproject_compact(oracle.median_u8(imgs[n - 1], 11), d2pc.make_q(), border=40, scale=0.125)
    assert res[2][2].view(np.uint32)[n - 1] == len(want)
    assert np.array_equal(res[2][1].view(np.uint32).reshape(n, -1)[n - 1][:len(wi)], wi)


@pytest.mark.parametrize("form", [1, 2])
def test_tile_fused_compact_kernel_is_capturable_and_runs_on_two_streams(form):
    """Captured without a warm-up call after d2pc_reserve_mono (its hand-off state is the capture's own), replayed
    onto wiped outputs; and two different batches in flight on two streams keep their own state."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 3, 300, 900
    rng = np.random.default_rng(21)
    sets = [_holey_images(rng, n, h, w, "iid"), _holey_images(rng, n, h, w, "blocky")]
    srcs = [torch.from_numpy(x).cuda() for x in sets]
    with d2pc.Context(q=q, mode=d2pc.MODE_COMPACT) as ctx:
        ctx.set_tuning("median_algo", 2)
        ctx.set_tuning("callback_fused_compact", form)
        bs = [DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True) for _ in range(2)]
        ctx.reserve_mono(d2pc.DTYPE_U8, w, h, n)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            ctx.process_mono_device(srcs[0].data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, bs[0].points.data_ptr(),
                                    bs[0].index.data_ptr(), bs[0].stride, bs[0].counts.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
        for _ in range(3):
            bs[0].points.fill_(0)
            bs[0].counts.fill_(0)
            torch.cuda.synchronize()
            g.replay()
            res = bs[0].results()
            ctx.check_async_error()
            for f in range(n):
                want, wi = oracle.reproject_compact(oracle.median_u8(sets[0][f], 11), q, border=40, scale=0.125)
                assert np.array_equal(res[f][1], wi)
                assert_points_close(res[f][0], want, max_ulp=1, what=f"replayed frame {f}")
        streams = [torch.cuda.Stream(), torch.cuda.Stream()]
        torch.cuda.synchronize()
        for _ in range(8):
            for src, b, s in zip(srcs, bs, streams):
                ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                        b.index.data_ptr(), b.stride, b.counts.data_ptr(), s.cuda_stream)
        torch.cuda.synchronize()
        ctx.check_async_error()
        for imgs, b in zip(sets, bs):
            res = b.results()
            for f in range(n):
                want, wi = oracle.reproject_compact(oracle.median_u8(imgs[f], 11), q, border=40, scale=0.125)
                assert np.array_equal(res[f][1], wi)
                assert_points_close(res[f][0], want, max_ulp=1, what=f"two-stream frame {f}")


def test_callback_body_compact_at_the_benchmark_size_one_kernel_equals_two_launches():
    """Config 4's geometry (16 x 3840x2160, 8-bit, ~30 % zero pixels in blocks): the one-kernel COMPACT callback body
    against the filter launch + compaction launch, compared on the device; two frames of it against the oracle."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    q = d2pc.make_q()
    n, h, w = 16, 2160, 3840
    g = torch.Generator(device="cuda").manual_seed(45)
    src = torch.randint(0, 256, (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
    holes = (torch.rand((n, (h + 63) // 64, (w + 63) // 64), device="cuda", generator=g) < 0.3)
    src[holes.repeat_interleave(64, dim=1).repeat_interleave(64, dim=2)[:, :h, :w]] = 0
    with d2pc.Context(q=q, mode=d2pc.MODE_COMPACT) as ctx:
        b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
        s = torch.cuda.current_stream().cuda_stream
        keep = {}
        for fused in (2, 1, 0):
            ctx.set_tuning("callback_fused_compact", fused)
            b.points.fill_(0)
            b.index.fill_(-1)
            b.counts.fill_(0)
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, 11, 0.125, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), s)
            torch.cuda.synchronize()
            ctx.check_async_error()
            keep[fused] = (b.points.view(torch.int32).clone(), b.index.clone(), b.counts.clone())
        for fused in (1, 2):
            for x, y in zip(keep[fused], keep[0]):
                assert torch.equal(x, y), f"form {fused}"
        res = b.results()
        st = ctx.compact_stats()
        assert st["timeouts"] == 0 and st["tiles"] >= 2 * 16 * 15 * 65
    imgs = src.cpu().numpy()
    for f in (0, 11):
        want, wi = oracle.reproject_compact(oracle.median_u8(imgs[f], 11), q, border=40, scale=0.125)
        assert 0.4 * 3760 * 2080 < len(want) < 0.9 * 3760 * 2080
        assert np.array_equal(res[f][1], wi)
        assert_points_close(res[f][0], want, max_ulp=1, what=f"frame {f}")
