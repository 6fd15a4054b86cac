"""The C-ABI session of the depth_map_fusion node (d2pc_fusion_node_*, through capi.FusionSession) against
colorize_ref.RefNode and the Python FusionNode: every published topic byte-equal after every callback, with the fusing
DisparityCb2 as ONE launch (single_launch = 1, d2pc_node.hip) and as the three-launch composition (0)."""
import ctypes

import numpy as np
import pytest
import torch

import disparity_to_point_cloud_amd as d2pc
from disparity_to_point_cloud_amd import capi
import oracle
import colorize_ref as ref
import value_patterns as vp
from test_colorize_cpu import node_inputs, structured

pytestmark = pytest.mark.gpu

CALLS = {"D1": "disparity_1", "D2": "disparity_2", "S1": "matching_score_1", "S2": "matching_score_2"}


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q()) as c:
        yield c


def _frames(seed, rows, cols, k=1):
    rng = np.random.default_rng(seed)
    out = {"D1": [], "D2": [], "S1": [], "S2": []}
    for _ in range(k):
        out["D1"].append(rng.integers(0, 256, size=(rows, cols)).astype(np.uint8))
        out["D2"].append(rng.integers(0, 256, size=(rows, cols)).astype(np.uint8))
        out["S1"].append((structured(rng, rows, cols) // 3).astype(np.uint8))
        out["S2"].append((structured(rng, rows, cols) // 3).astype(np.uint8))
    return out


class Trio:
    """The C session with and without the single launch, the Python session and the model, stepped together."""

    def __init__(self, ctx, cols, rows, ox=0, oy=0, **kw):
        self.one = d2pc.FusionSession(ctx, cols, rows, ox, oy, single_launch=1, **kw)
        self.three = d2pc.FusionSession(ctx, cols, rows, ox, oy, single_launch=0, **kw)
        self.py = d2pc.FusionNode(ctx, cols, rows, ox, oy, **kw)
        self.model = ref.RefNode(cols, rows, ox, oy, rule=kw.get("rule", oracle.FUSE_GRAD_FILTER), form=kw.get("form", 4))
        assert self.one.cfg.single_launch == 1 and self.three.cfg.single_launch == 0

    def step(self, call, frame, what=""):
        d = torch.from_numpy(frame).cuda()
        got = [getattr(s, CALLS[call])(d) for s in (self.one, self.three, self.py)]
        torch.cuda.synchronize()
        want = getattr(self.model, CALLS[call])(frame)
        for name, g in zip(("single launch", "three launches", "FusionNode"), got):
            assert g.keys() == want.keys(), (what, call, name, sorted(g), sorted(want))
            for topic, w in want.items():
                a = g[topic].cpu().numpy()
                assert a.shape == w.shape, (what, call, name, topic, a.shape, w.shape)
                assert np.array_equal(a, w), (what, call, name, topic, int((a != w).sum()))
        for topic in want:
            assert torch.equal(got[0][topic], got[1][topic]) and torch.equal(got[0][topic], got[2][topic]), (what, call, topic)
        return got[0], want

    def close(self):
        self.one.close(), self.three.close()


def _run(ctx, cols, rows, ox, oy, order, seed=1, **kw):
    t = Trio(ctx, cols, rows, ox, oy, **kw)
    fr = _frames(seed, rows, cols, k=len(order))
    outs = [t.step(call, fr[call][i], (cols, rows, ox, oy, i)) for i, call in enumerate(order)]
    return t, outs


def test_reference_geometry(ctx):
    t, outs = _run(ctx, 752, 480, -7, 15, ["D1", "S1", "S2", "D2"])
    assert t.one.n == 465 and t.one.sq1 == t.model.sq1 and t.one.sq2 == t.model.sq2
    got = outs[-1][0]
    assert tuple(got["cropped_depth_2"].shape) == (465, 465, 3) and tuple(got["combined_score"].shape) == (465, 465)
    assert tuple(got["gradient"].shape) == (425, 425, 3) and tuple(got["fused_depth_map"].shape) == (425, 425)
    assert (got["fused_depth_map"] > 0).any()
    t.close()


@pytest.mark.parametrize("cols,rows,ox,oy", [(188, 120, 0, 0), (120, 188, 3, -5), (160, 160, -4, 9)])
def test_zero_offsets_portrait_and_square(ctx, cols, rows, ox, oy):
    _run(ctx, cols, rows, ox, oy, ["S1", "D1", "S2", "D2"], seed=cols + oy)[0].close()


def test_camera_2_negated_offsets_and_member_offset_y(ctx):
    s = d2pc.FusionSession(ctx, 752, 480, -7, 15)
    assert s.sq1 == oracle.crop_to_square(752, 480, -7, 15)
    assert s.sq2 == oracle.crop_to_square(480, 752, 7, -15, 15)
    assert s.sq2 != oracle.crop_to_square(480, 752, -7, 15, 15)
    s.close()
    _run(ctx, 200, 140, 6, -9, ["D2", "D1", "S2", "S1", "D2"], seed=3)[0].close()


def test_fusion_withheld_until_the_fourth_plane(ctx):
    t, outs = _run(ctx, 188, 120, -2, 4, ["D2", "S1", "D2", "D1", "D2", "S2", "D2"], seed=4)
    keys = [sorted(o[0]) for o in outs]
    assert keys[0] == keys[2] == keys[4] == ["cropped_depth_2"]
    assert keys[6] == ["combined_score", "cropped_depth_2", "fused_depth_map", "gradient"]
    t.close()


def test_second_fusion_sees_the_overwritten_score(ctx):
    disp, score = node_inputs()
    t = Trio(ctx, 188, 120, -2, 4)
    t.step("D1", disp[0]), t.step("S1", score[0]), t.step("S2", score[1])
    first, wfirst = t.step("D2", disp[1])
    first_fused = first["fused_depth_map"].cpu().numpy().copy()
    second, wsecond = t.step("D2", disp[1])
    assert (second["fused_depth_map"].cpu().numpy() != first_fused).any()
    assert (wsecond["fused_depth_map"] != wfirst["fused_depth_map"]).any()
    # no copy: the combined plane IS camera 1's score plane now, and it is the other buffer of the first fusion
    s1 = t.step("S1", score[0])[0]  # S1 between two D2 restores camera 1's score
    assert s1["cropped_score_1"].data_ptr() == second["combined_score"].data_ptr() != first["combined_score"].data_ptr()
    third, _ = t.step("D2", disp[1])
    assert np.array_equal(third["fused_depth_map"].cpu().numpy(), first_fused)
    t.close()


def test_twenty_interleaved_callbacks(ctx):
    rng = np.random.default_rng(20)
    order = [["D1", "D2", "S1", "S2"][i] for i in rng.integers(0, 4, size=20)]
    assert len(set(order)) == 4
    _run(ctx, 170, 130, 3, 5, order, seed=21)[0].close()


def test_form_cv3_and_another_rule(ctx):
    _run(ctx, 188, 120, -2, 4, ["D1", "S1", "S2", "D2", "D2"], seed=5, form=d2pc.SCORE_FORM_CV3)[0].close()
    # a rule without a single-launch kernel takes the composition inside the same session, whatever single_launch says
    _run(ctx, 188, 120, -2, 4, ["D1", "S1", "S2", "D2"], seed=6, rule=d2pc.FUSE_BETTER_SCORE)[0].close()


@pytest.mark.parametrize("single", [1, 0])
def test_batch_of_three_equals_three_sessions(ctx, single):
    cols, rows, ox, oy = 188, 120, -2, 4
    order = ["D1", "S1", "S2", "D2", "D2", "S1", "D2"]
    fr = [_frames(30 + k, rows, cols, k=len(order)) for k in range(3)]
    batch = d2pc.FusionSession(ctx, cols, rows, ox, oy, batch=3, single_launch=single)
    single_s = [d2pc.FusionSession(ctx, cols, rows, ox, oy, single_launch=single) for _ in range(3)]
    models = [ref.RefNode(cols, rows, ox, oy) for _ in range(3)]
    for i, call in enumerate(order):
        stack = torch.from_numpy(np.stack([fr[k][call][i] for k in range(3)])).cuda()
        got = getattr(batch, CALLS[call])(stack)
        torch.cuda.synchronize()
        for k in range(3):
            one = getattr(single_s[k], CALLS[call])(stack[k])
            want = getattr(models[k], CALLS[call])(fr[k][call][i])
            torch.cuda.synchronize()
            assert got.keys() == one.keys() == want.keys()
            for topic in want:
                assert torch.equal(got[topic][k], one[topic]), (i, call, k, topic)
                assert np.array_equal(got[topic][k].cpu().numpy(), want[topic]), (i, call, k, topic)


# ---- the single-launch kernel on chosen values ---------------------------------------------------------------------
def _frame_for_view_2(sess, plane, fill, batch_shape=()):
    """A raw camera-2 frame whose rotated, cropped view is `plane` (..., n, n)."""
    x, y, n = sess.sq2
    rot = np.full(batch_shape + (sess.cols, sess.rows), fill, dtype=np.uint8)  # the rotated frame: cols rows of `rows` pixels
    rot[..., y:y + n, x:x + n] = plane
    return np.ascontiguousarray(np.rot90(rot, 1, axes=(-2, -1)))  # oracle.rotate_cw is rot90(., -1)


def _frame_for_view_1(sess, plane, fill, batch_shape=()):
    x, y, n = sess.sq1
    fr = np.full(batch_shape + (sess.rows, sess.cols), fill, dtype=np.uint8)
    fr[..., y:y + n, x:x + n] = plane
    return fr


def _fuse_planes(ctx, cols, rows, ox, oy, d1, d2, s1, s2, batch=1, crop=None, pad=0, shift=0):
    """Put the four n x n planes (batch, n, n) into sessions with and without the single launch (the score planes
    through the writable views the score callbacks return), run the fusing DisparityCb2 on a camera-2 frame with rows
    `pad` bytes longer than the width and a base address `shift` bytes off, and compare all four topics with the
    oracle's fuse + the colouring."""
    crop = crop or ref.RefNode.CROP
    outs = []
    for single in (1, 0):
        s = d2pc.FusionSession(ctx, cols, rows, ox, oy, batch=batch, single_launch=single, crop=crop)
        n = s.n
        assert d1.shape == (batch, n, n)
        bs = (batch,) if batch > 1 else ()
        sh = (lambda a: a if batch > 1 else a[0])
        zero = torch.zeros(bs + (rows, cols), dtype=torch.uint8, device="cuda")
        s.disparity_1(torch.from_numpy(_frame_for_view_1(s, sh(d1), 7, bs)).cuda())
        s.matching_score_1(zero)["cropped_score_1"].copy_(torch.from_numpy(sh(s1)))
        s.matching_score_2(zero)["cropped_score_2"].copy_(torch.from_numpy(sh(s2)))
        f2 = _frame_for_view_2(s, sh(d2), 9, bs)
        # pitch > width and a base address offset by 1..3 bytes
        store = torch.zeros(batch * rows * (cols + pad) + 8, dtype=torch.uint8, device="cuda")
        dev = store[shift:shift + batch * rows * (cols + pad)].view(bs + (rows, cols + pad))[..., :cols]
        dev.copy_(torch.from_numpy(f2))
        assert dev.data_ptr() % 4 == shift % 4 and dev.stride(-2) == cols + pad
        got = s.disparity_2(dev)
        torch.cuda.synchronize()
        assert sorted(got) == ["combined_score", "cropped_depth_2", "fused_depth_map", "gradient"]
        got = {k: (v if batch > 1 else v[None]).cpu().numpy() for k, v in got.items()}
        for b in range(batch):
            fused, comb = oracle.fuse([np.ascontiguousarray(p[b]) for p in (d1, d2, s1, s2, s1, s2)],
                                      rule=oracle.FUSE_GRAD_FILTER, crop=crop)
            want = {"cropped_depth_2": ref.colorize(d2[b]), "combined_score": comb, "fused_depth_map": fused,
                    "gradient": ref.colorize(fused)}
            for topic, w in want.items():
                g = got[topic][b]
                assert g.shape == w.shape, (single, topic, g.shape, w.shape)
                assert np.array_equal(g, w), (single, b, topic, int((g != w).sum()), np.argwhere(g != w)[:4].tolist())
        outs.append(got)
        s.close()
    for topic in outs[0]:
        assert np.array_equal(outs[0][topic], outs[1][topic]), topic
    return outs[0]


def _boundary_planes(rng, n):
    """d1, d2, s1, s2 on every branch boundary of gradFilter (:214-235): scores at and one off 100 and 125 and equal
    to each other, depths at and one off 230, d1 / d2 on and next to 4/5 and 5/4, d2 = 0."""
    edge_s = np.array([0, 1, 99, 100, 101, 124, 125, 126, 254, 255])
    edge_d = np.array([0, 1, 4, 5, 8, 10, 100, 125, 80, 99, 101, 124, 126, 229, 230, 231, 184, 183, 185, 255, 204, 203, 205])
    d2 = rng.choice(edge_d, size=(n, n))
    ratio = rng.integers(0, 6, size=(n, n))
    d1 = rng.choice(edge_d, size=(n, n))
    on45 = (d2 % 5 == 0) & (ratio == 0)       # d1 = 4/5 d2 exactly (passes), and one below (fails)
    d1 = np.where(on45, d2 // 5 * 4, d1)
    d1 = np.where((d2 % 5 == 0) & (ratio == 1), np.maximum(d2 // 5 * 4 - 1, 0), d1)
    on54 = (d2 % 4 == 0) & (d2 <= 204) & (ratio == 2)   # d1 = 5/4 d2 exactly (fails), and one below (passes)
    d1 = np.where(on54, d2 // 4 * 5, d1)
    d1 = np.where((d2 % 4 == 0) & (d2 <= 204) & (ratio == 3), np.maximum(d2 // 4 * 5 - 1, 0), d1)
    s1 = rng.choice(edge_s, size=(n, n))
    s2 = np.where(rng.random((n, n)) < 0.25, s1, rng.choice(edge_s, size=(n, n)))
    assert on45.any() and on54.any() and (d2 == 0).any() and (s1 == s2).any()
    return [p.astype(np.uint8)[None] for p in (d1, d2, s1, s2)]


def test_every_branch_boundary_of_grad_filter(ctx):
    s = d2pc.FusionSession(ctx, 188, 120, -2, 4)
    n = s.n
    s.close()
    d1, d2, s1, s2 = _boundary_planes(np.random.default_rng(50), n)
    got = _fuse_planes(ctx, 188, 120, -2, 4, d1, d2, s1, s2)
    # all three outcomes occur: camera 1's depth, camera 2's, the average, and black
    f = got["fused_depth_map"]
    assert (f == 0).any() and (f > 0).any()
    # whole byte range, sparse and dense (value_patterns): medians near both ends of the table
    rng = np.random.default_rng(51)
    full = [rng.integers(0, 256, size=(1, n, n)).astype(np.uint8) for _ in range(4)]
    _fuse_planes(ctx, 188, 120, -2, 4, *full)
    bands = [vp.narrow_band(rng, n, n, lo, w)[None] for lo, w in ((0, 4), (252, 4), (96, 8), (120, 8))]
    _fuse_planes(ctx, 188, 120, -2, 4, bands[1], bands[1], bands[2], bands[3])
    _fuse_planes(ctx, 188, 120, -2, 4, bands[0], bands[1], bands[0], bands[0])
    two = [vp.two_level(rng, n, n, lo, hi, k=3)[None] for lo, hi in ((127, 128), (0, 255), (99, 100), (124, 125))]
    _fuse_planes(ctx, 188, 120, -2, 4, two[0], two[1], two[2], two[3])


def test_constant_and_checkerboard_frames(ctx):
    s = d2pc.FusionSession(ctx, 188, 120, -2, 4)
    n = s.n
    s.close()
    yy, xx = np.mgrid[0:n, 0:n]
    board = np.where((yy + xx) % 2 == 0, 200, 10).astype(np.uint8)[None]
    rows_ = np.where(yy % 2 == 0, 180, 20).astype(np.uint8)[None]
    const = lambda v: np.full((1, n, n), v, dtype=np.uint8)  # noqa: E731
    # camera 1 wins everywhere (s1 < s2, s1 < 100, d1 < 230): the fused image is d1, so the median sees the pattern
    for d1 in (const(0), const(255), const(77), board, rows_, 255 - board):
        _fuse_planes(ctx, 188, 120, -2, 4, d1, const(50), const(10), const(90))
    _fuse_planes(ctx, 188, 120, -2, 4, const(50), board, const(90), const(10))   # camera 2 wins
    _fuse_planes(ctx, 188, 120, -2, 4, board, board, board, 255 - board)         # the winner alternates per pixel


@pytest.mark.parametrize("cols,rows,ox,oy,crop", [
    (11, 11, 0, 0, (0, 4, 3, 1)),        # n = 11, the smallest square
    (11, 40, 0, 0, (2, 2, 2, 2)),        # portrait, n = 11
    (77, 90, 2, -3, (0, 40, 30, 10)),    # n = 74: not a multiple of 4
    (41, 41, 0, 0, (0, 40, 30, 10)),     # n = 41: a fused map 1 pixel wide
    (130, 67, 0, 0, (64, 2, 0, 66)),     # n = 67: a 1 x 1 fused map, on a tile's first column
    (131, 131, 0, 0, (63, 3, 15, 17)),   # n = 131: three tiles across, the crop starts on a tile's last column
])
def test_small_and_odd_squares(ctx, cols, rows, ox, oy, crop):
    s = d2pc.FusionSession(ctx, cols, rows, ox, oy, crop=crop)
    n = s.n
    s.close()
    rng = np.random.default_rng(60 + cols)
    planes = [rng.integers(0, 256, size=(1, n, n)).astype(np.uint8) for _ in range(2)] + \
             [rng.integers(60, 140, size=(1, n, n)).astype(np.uint8) for _ in range(2)]
    got = _fuse_planes(ctx, cols, rows, ox, oy, *planes, crop=crop)
    assert got["fused_depth_map"].shape[1:] == (n - crop[2] - crop[3], n - crop[0] - crop[1])


@pytest.mark.parametrize("pad,shift", [(0, 1), (5, 2), (19, 3), (64, 0)])
def test_pitches_and_unaligned_bases(ctx, pad, shift):
    s = d2pc.FusionSession(ctx, 188, 120, -2, 4)
    n = s.n
    s.close()
    rng = np.random.default_rng(70 + pad)
    planes = [rng.integers(0, 256, size=(1, n, n)).astype(np.uint8) for _ in range(2)] + \
             [rng.integers(60, 140, size=(1, n, n)).astype(np.uint8) for _ in range(2)]
    _fuse_planes(ctx, 188, 120, -2, 4, *planes, pad=pad, shift=shift)


def test_batch_of_sixteen(ctx):
    s = d2pc.FusionSession(ctx, 200, 150, 2, -3)
    n = s.n
    s.close()
    rng = np.random.default_rng(80)
    planes = [rng.integers(0, 256, size=(16, n, n)).astype(np.uint8) for _ in range(2)] + \
             [rng.integers(60, 140, size=(16, n, n)).astype(np.uint8) for _ in range(2)]
    _fuse_planes(ctx, 200, 150, 2, -3, *planes, batch=16, pad=8, shift=1)
    # ... and a batch large enough for the tall tiles (2048 tiles of 64 x 64): 16 frames of n = 736
    s = d2pc.FusionSession(ctx, 740, 736, 0, 0)
    n = s.n
    s.close()
    assert (-(-n // 64)) ** 2 * 16 >= 2048
    planes = [rng.integers(0, 256, size=(16, n, n)).astype(np.uint8) for _ in range(2)] + \
             [rng.integers(60, 140, size=(16, n, n)).astype(np.uint8) for _ in range(2)]
    _fuse_planes(ctx, 740, 736, 0, 0, *planes, batch=16)


# ---- graph capture --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("single", [1, 0])
def test_captured_pair_replays_on_new_frames(ctx, single):
    """MATCHING_SCORE_1 + DISPARITY_2 through d2pc_fusion_node_callback_device, captured as one graph (one stream, a
    linear chain: no parallel branches) and replayed on new frame contents, against an eager session and the model."""
    cols, rows, ox, oy = 752, 480, -7, 15
    fr = _frames(40, rows, cols, k=4)
    node, eager = (d2pc.FusionSession(ctx, cols, rows, ox, oy, single_launch=single) for _ in range(2))
    model = ref.RefNode(cols, rows, ox, oy)
    static_d2, static_s1 = torch.from_numpy(fr["D2"][0]).cuda(), torch.from_numpy(fr["S1"][0]).cuda()
    for n in (node, eager):
        n.disparity_1(torch.from_numpy(fr["D1"][0]).cuda())
        n.matching_score_2(torch.from_numpy(fr["S2"][0]).cuda())
    model.disparity_1(fr["D1"][0]), model.matching_score_2(fr["S2"][0])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):  # warm-up outside the capture
        node.matching_score_1(static_s1)
        node.disparity_2(static_d2)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        topics = dict(node.matching_score_1(static_s1))
        topics.update(node.disparity_2(static_d2))
    assert len(topics) == 5
    for rep in range(1, 4):
        static_s1.copy_(torch.from_numpy(fr["S1"][rep]))
        static_d2.copy_(torch.from_numpy(fr["D2"][rep]))
        g.replay()
        torch.cuda.synchronize()
        want = dict(model.matching_score_1(fr["S1"][rep]))
        del want["cropped_score_1"]  # its plane has been fused over since (:113); the eager tensor below likewise
        want.update(model.disparity_2(fr["D2"][rep]))
        eager.matching_score_1(static_s1)
        got = eager.disparity_2(static_d2)
        torch.cuda.synchronize()
        for topic, w in want.items():
            assert np.array_equal(topics[topic].cpu().numpy(), w), (rep, topic)
            assert torch.equal(topics[topic], got[topic]), (rep, topic)
    node.close(), eager.close()


# ---- arguments ------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_node_alive(ctx):
    lib = d2pc.load_library()
    s = d2pc.FusionSession(ctx, 188, 120, -2, 4)
    ok = torch.zeros((120, 188), dtype=torch.uint8, device="cuda")
    out = capi.FusionNodeTopics()
    out.struct_size = ctypes.sizeof(out)
    call = lib.d2pc_fusion_node_callback_device
    assert call(s._h, 4, ok.data_ptr(), 188, 0, ctypes.byref(out), None) == 1      # bad `which`
    assert call(s._h, -1, ok.data_ptr(), 188, 0, ctypes.byref(out), None) == 1
    assert call(s._h, 0, None, 188, 0, ctypes.byref(out), None) == 1              # null frame
    assert call(s._h, 0, ok.data_ptr(), 188, 0, None, None) == 1                  # null topics
    assert call(s._h, 0, ok.data_ptr(), 187, 0, ctypes.byref(out), None) == 3     # pitch < cols
    assert call(s._h, 0, ok.data_ptr(), 1 << 32, 0, ctypes.byref(out), None) == 3  # pitch >= 2^32
    assert call(s._h, 4, ok.data_ptr(), 187, 0, ctypes.byref(out), None) == 1     # two faults: `which` comes first,
    assert call(s._h, 0, None, 187, 0, ctypes.byref(out), None) == 1              # ... and so does the null frame
    with d2pc.FusionSession(ctx, 188, 120, -2, 4, batch=2) as s2:                 # a batch: the frame stride counts
        two = torch.zeros((2, 120, 188), dtype=torch.uint8, device="cuda")
        assert call(s2._h, 0, two.data_ptr(), 188, 119 * 188 + 187, ctypes.byref(out), None) == 3
        assert call(s2._h, 4, two.data_ptr(), 188, 119 * 188 + 187, ctypes.byref(out), None) == 1
        assert call(s2._h, 0, two.data_ptr(), 188, 119 * 188 + 188, ctypes.byref(out), None) == 0
    out.struct_size = 8
    assert call(s._h, 0, ok.data_ptr(), 188, 0, ctypes.byref(out), None) == 1
    junk = (ctypes.c_uint8 * 512)()                                               # not a node
    out.struct_size = ctypes.sizeof(out)
    assert call(ctypes.addressof(junk), 0, ok.data_ptr(), 188, 0, ctypes.byref(out), None) == 1
    assert lib.d2pc_fusion_node_destroy(ctypes.addressof(junk)) == 1
    for bad in (torch.zeros((188, 120), dtype=torch.uint8, device="cuda"), torch.zeros((120, 188), dtype=torch.int16, device="cuda"),
                torch.zeros((120, 188), dtype=torch.uint8), np.zeros((120, 188), dtype=np.uint8)):
        with pytest.raises(ValueError):
            s.disparity_1(bad)
    with pytest.raises(d2pc.D2pcError) as e:
        d2pc.FusionSession(ctx, 188, 120, 0, 0, crop=(0, 120, 0, 0))              # nothing left of the fused map
    assert e.value.status == 3
    with pytest.raises(d2pc.D2pcError):
        d2pc.FusionSession(ctx, 188, 120, batch=0)
    assert sorted(s.disparity_1(ok)) == ["cropped_depth_1"]                       # the node lives on
    s.close()
