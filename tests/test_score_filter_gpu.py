"""d2pc_score_filter_device on the GPU, bit for bit against the integer restatement tests/score_filter_ref.py
(DESIGN.md section 8a): both directions and forms, the edges of frame and square, batches with strides and views,
misuse, graph capture, 4K batches and the whole depth_map_fusion node on the device."""
import ctypes

import numpy as np
import pytest
import torch

import disparity_to_point_cloud_amd as d2pc
import oracle
import score_filter_ref as ref
from disparity_to_point_cloud_amd.torch_api import fuse_planes, score_filter

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q()) as c:
        yield c


def _structured(rng, h, w):
    """Blocky frames with noise: the threshold goes both ways (random noise alone blurs to nearly flat)."""
    base = rng.integers(0, 256, size=(h // 9 + 2, w // 9 + 2)).astype(np.float64)
    f = np.kron(base, np.ones((9, 9)))[:h, :w]
    return np.clip(f + rng.integers(-25, 26, size=(h, w)), 0, 255).astype(np.uint8)


def _check(ctx, frame, sq, direction, form, want_grad=True):
    got_o, got_g = score_filter(ctx, torch.from_numpy(frame).cuda(), sq, direction, form, want_grad=want_grad)
    torch.cuda.synchronize()
    want_o, want_g = ref.score_filter(frame, sq, direction, form)
    assert np.array_equal(got_o.cpu().numpy(), want_o), (frame.shape, sq, direction, form)
    if want_grad:
        assert np.array_equal(got_g.cpu().numpy(), want_g), (frame.shape, sq, direction, form)
    else:
        assert got_g is None
    return want_g


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("form", [d2pc.SCORE_FORM_CV4, d2pc.SCORE_FORM_CV3])
def test_random_and_structured_frames(ctx, direction, form):
    rng = np.random.default_rng(10 * direction + form)
    hit = 0
    for h, w, sq in ((480, 752, d2pc.crop_to_square(752, 480, -7, 15)), (200, 150, (3, 30, 141)), (97, 131, (17, 0, 97))):
        for frame in (rng.integers(0, 256, size=(h, w)).astype(np.uint8), _structured(rng, h, w)):
            for want_grad in (True, False):
                g = _check(ctx, frame, sq, direction, form, want_grad)
                hit += int(g.max() > 0)
    assert hit > 0  # the threshold fired somewhere


@pytest.mark.parametrize("h,w", [(11, 11), (11, 40), (40, 11), (13, 12), (63, 65), (65, 63), (300, 77), (77, 300)])
def test_small_odd_tall_and_landscape(ctx, h, w):
    rng = np.random.default_rng(h * 1000 + w)
    frame = _structured(rng, h, w)
    n = min(h, w)
    for sq in ((0, 0, n), (w - n, h - n, n), ((w - n) // 2, (h - n) // 2, n)):
        for direction in (0, 1):
            _check(ctx, frame, sq, direction, 4)
    if n >= 12:
        _check(ctx, frame, (w - 11, h - 11, 11), 1, 3)  # n = 11 in the far corner


def test_squares_at_every_frame_edge(ctx):
    """G13 reflects about the frame, the rest about the square: squares flush with each edge, corner and none,
    with n across the 32 / 64 tile boundaries."""
    rng = np.random.default_rng(5)
    h, w = 150, 170
    frame = _structured(rng, h, w)
    for n in (11, 31, 32, 33, 64, 65, 97, 128, 129, 150):
        for x in sorted({0, 1, 6, (w - n) // 2, w - n - 6, w - n - 1, w - n}):
            for y in sorted({0, 1, 6, (h - n) // 2, h - n - 1, h - n}):
                if 0 <= x <= w - n and 0 <= y <= h - n:
                    _check(ctx, frame, (x, y, n), (x + y + n) & 1, 4 if n & 2 else 3)


def test_batches_pitches_and_views(ctx):
    rng = np.random.default_rng(9)
    f, h, w = 5, 120, 200
    big = torch.from_numpy(np.stack([_structured(rng, h + 7, w + 13) for _ in range(f + 2)])).cuda()
    view = big[1:1 + f, 3:3 + h, 5:5 + w]  # row pitch w + 13, frame stride (h + 7)(w + 13), offset origin
    host = view.cpu().numpy()
    sq = (40, 4, 112)
    for direction, form in ((0, 4), (1, 3)):
        out, grad = score_filter(ctx, view, sq, direction, form, want_grad=True)
        torch.cuda.synchronize()
        for k in range(f):
            wo, wg = ref.score_filter(host[k], sq, direction, form)
            assert np.array_equal(out[k].cpu().numpy(), wo), k
            assert np.array_equal(grad[k].cpu().numpy(), wg), k
    # strided outputs through the C ABI directly: out and grad rows padded, frames padded
    n = sq[2]
    po, pg = n + 9, n + 3
    out = torch.full((f, n + 2, po), 7, dtype=torch.uint8, device="cuda")
    grad = torch.full((f, n + 1, pg), 7, dtype=torch.uint8, device="cuda")
    d = d2pc.score_filter_desc_init()
    d.direction, d.width, d.height, d.n_frames = 1, w, h, f
    d.x, d.y, d.n = sq
    d.src, d.src_pitch, d.src_frame_stride = view.data_ptr(), view.stride(1), view.stride(0)
    d.out, d.out_pitch, d.out_frame_stride = out.data_ptr(), po, (n + 2) * po
    d.grad, d.grad_pitch, d.grad_frame_stride = grad.data_ptr(), pg, (n + 1) * pg
    ctx.score_filter_device(d, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    o, g = out.cpu().numpy(), grad.cpu().numpy()
    for k in range(f):
        wo, wg = ref.score_filter(host[k], sq, 1, 4)
        assert np.array_equal(o[k, :n, :n], wo) and np.array_equal(g[k, :n, :n], wg), k
    assert (o[:, :n, n:] == 7).all() and (o[:, n:] == 7).all() and (g[:, :n, n:] == 7).all() and (g[:, n:] == 7).all()


def test_misuse_returns_codes_without_launching(ctx):
    h, w, n = 64, 80, 50
    src = torch.zeros((2, h, w), dtype=torch.uint8, device="cuda")
    out = torch.full((2, n, n), 99, dtype=torch.uint8, device="cuda")
    grad = torch.full((2, n, n), 99, dtype=torch.uint8, device="cuda")
    lib = d2pc.load_library()

    def good():
        d = d2pc.score_filter_desc_init()
        d.width, d.height, d.n_frames, d.x, d.y, d.n = w, h, 2, 10, 5, n
        d.src, d.src_pitch, d.src_frame_stride = src.data_ptr(), w, w * h
        d.out, d.out_pitch, d.out_frame_stride = out.data_ptr(), n, n * n
        d.grad, d.grad_pitch, d.grad_frame_stride = grad.data_ptr(), n, n * n
        return d

    INV, SIZE = 1, 3
    cases = [
        ("struct_size", lambda d: setattr(d, "struct_size", 12), INV),
        ("direction", lambda d: setattr(d, "direction", 2), INV),
        ("direction<0", lambda d: setattr(d, "direction", -1), INV),
        ("form", lambda d: setattr(d, "form", 5), INV),
        ("n<11", lambda d: setattr(d, "n", 10), SIZE),
        ("x<0", lambda d: setattr(d, "x", -1), SIZE),
        ("outside x", lambda d: setattr(d, "x", w - n + 1), SIZE),
        ("outside y", lambda d: setattr(d, "y", h - n + 1), SIZE),
        ("frames", lambda d: setattr(d, "n_frames", 0), SIZE),
        ("src pitch", lambda d: setattr(d, "src_pitch", w - 1), SIZE),
        ("src frame stride", lambda d: setattr(d, "src_frame_stride", w * h - 1), SIZE),
        ("plane >= 4 GiB", lambda d: setattr(d, "src_pitch", 1 << 27), SIZE),
        ("out pitch", lambda d: setattr(d, "out_pitch", n - 1), SIZE),
        ("out frame stride", lambda d: setattr(d, "out_frame_stride", n * n - 1), SIZE),
        ("grad pitch", lambda d: setattr(d, "grad_pitch", n - 1), SIZE),
        ("null src", lambda d: setattr(d, "src", None), INV),
        ("null out", lambda d: setattr(d, "out", None), INV),
        ("in place", lambda d: setattr(d, "out", src.data_ptr() + 100), INV),
        ("grad on src", lambda d: setattr(d, "grad", src.data_ptr()), INV),
        ("grad on out", lambda d: setattr(d, "grad", out.data_ptr() + n), INV),
        # two faults at once: the order of the checks decides the code -- direction and form, the sizes and the square,
        # then the pointers, then the planes (source, out, grad), then the overlaps
        ("direction + frames", lambda d: (setattr(d, "direction", 2), setattr(d, "n_frames", 0)), INV),
        ("n<11 + null src", lambda d: (setattr(d, "n", 10), setattr(d, "src", None)), SIZE),
        ("src pitch + null out", lambda d: (setattr(d, "src_pitch", w - 1), setattr(d, "out", None)), INV),
        ("out pitch + in place", lambda d: (setattr(d, "out_pitch", n - 1), setattr(d, "out", src.data_ptr() + 100)), SIZE),
        ("grad frame stride + grad on src",
         lambda d: (setattr(d, "grad_frame_stride", n * n - 1), setattr(d, "grad", src.data_ptr())), SIZE),
    ]
    for name, mutate, code in cases:
        d = good()
        mutate(d)
        st = lib.d2pc_score_filter_device(ctx._h, ctypes.byref(d), None)
        assert st == code, (name, st)
    assert lib.d2pc_score_filter_device(ctx._h, None, None) == INV
    assert lib.d2pc_score_filter_device(None, ctypes.byref(good()), None) == INV
    torch.cuda.synchronize()
    assert (out == 99).all() and (grad == 99).all()  # nothing launched
    # and the good descriptor does run
    st = lib.d2pc_score_filter_device(ctx._h, ctypes.byref(good()), None)
    torch.cuda.synchronize()
    assert st == 0 and (out == 0).all() and (grad == 0).all()


def test_graph_capture_and_replay(ctx):
    rng = np.random.default_rng(3)
    h, w = 480, 752
    sq = d2pc.crop_to_square(w, h, -7, 15)
    static = torch.from_numpy(np.stack([_structured(rng, h, w) for _ in range(2)])).cuda()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        score_filter(ctx, static, sq, 0, 4, want_grad=True)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out, grad = score_filter(ctx, static, sq, 0, 4, want_grad=True)
    for rep in range(3):
        frames = np.stack([_structured(rng, h, w) for _ in range(2)])
        static.copy_(torch.from_numpy(frames))
        g.replay()
        torch.cuda.synchronize()
        for k in range(2):
            wo, wg = ref.score_filter(frames[k], sq, 0, 4)
            assert np.array_equal(out[k].cpu().numpy(), wo), (rep, k)
            assert np.array_equal(grad[k].cpu().numpy(), wg), (rep, k)


def test_4k_batch_sampled(ctx):
    """16 x 3840 x 2160 (n = 2160, the 64-pixel tiles), checked on three sampled frames."""
    rng = np.random.default_rng(4)
    f, h, w = 16, 2160, 3840
    frames = torch.randint(0, 256, (f, h, w), dtype=torch.uint8, device="cuda")
    # blocky content in the sampled frames so that the threshold fires
    sample = (0, 7, 15)
    for k in sample:
        frames[k] = torch.from_numpy(_structured(rng, h, w)).cuda()
    sq = d2pc.crop_to_square(w, h)
    assert sq[2] == 2160
    for direction, form in ((0, 4), (1, 3)):
        out, grad = score_filter(ctx, frames, sq, direction, form, want_grad=True)
        torch.cuda.synchronize()
        for k in sample[:2] if direction else sample[1:]:
            wo, wg = ref.score_filter(frames[k].cpu().numpy(), sq, direction, form)
            assert np.array_equal(out[k].cpu().numpy(), wo), (direction, k)
            assert np.array_equal(grad[k].cpu().numpy(), wg), (direction, k)


def test_whole_fusion_node_on_device(ctx):
    """depth_map_fusion end to end on the device: four raw 752 x 480 planes (disparity and matching score of both
    cameras) -> rotate camera 2 -> crop to square -> score filter per camera -> fuse, with the filtered score in
    both the score and the grad slot as the reference does (src/depth_map_fusion.cpp:77,96)."""
    rng = np.random.default_rng(78)
    H, W, ox, oy = 480, 752, -7, 15
    raw = [rng.integers(0, 256, size=(H, W)).astype(np.uint8) for _ in range(2)] + \
          [_structured(rng, H, W) for _ in range(2)]  # disp1, disp2, score1, score2
    x1, y1, n = oracle.crop_to_square(W, H, ox, oy)
    x2, y2, n2 = oracle.crop_to_square(H, W, -ox, -oy, oy)
    assert n == n2 == 465
    d1 = raw[0][y1:y1 + n, x1:x1 + n]
    d2_ = oracle.rotate_cw(raw[1])[y2:y2 + n, x2:x2 + n]
    o1, _ = ref.score_filter(raw[2], (x1, y1, n), 0, 4)
    o2, _ = ref.score_filter(oracle.rotate_cw(raw[3]), (x2, y2, n), 1, 4)
    want_f, want_c = oracle.fuse([np.ascontiguousarray(p) for p in (d1, d2_, o1, o2, o1, o2)])
    dev = [torch.from_numpy(r).cuda() for r in raw]
    rot = [torch.empty((W, H), dtype=torch.uint8, device="cuda") for _ in range(2)]
    stream = torch.cuda.current_stream().cuda_stream
    for src, dst in ((dev[1], rot[0]), (dev[3], rot[1])):
        ctx.rotate_cw_device(src.data_ptr(), W, H, W, 0, 1, dst.data_ptr(), H, 0, stream)
    sq1 = d2pc.crop_to_square(W, H, ox, oy)
    sq2 = d2pc.crop_to_square(H, W, -ox, -oy, oy)
    s1, _ = score_filter(ctx, dev[2], sq1, 0)
    s2, _ = score_filter(ctx, rot[1], sq2, 1)
    cx1, cy1, cn = sq1
    cx2, cy2, _ = sq2
    planes = [dev[0][cy1:cy1 + cn, cx1:cx1 + cn], rot[0][cy2:cy2 + cn, cx2:cx2 + cn], s1, s2, s1, s2]
    fused, comb = fuse_planes(ctx, planes)
    torch.cuda.synchronize()
    assert np.array_equal(s1.cpu().numpy(), o1) and np.array_equal(s2.cpu().numpy(), o2)
    assert np.array_equal(fused.cpu().numpy(), want_f)
    assert np.array_equal(comb.cpu().numpy(), want_c)
