"""FusionNode (the depth_map_fusion node as a device session) against colorize_ref.RefNode, the reference's sequence
of statements on numpy arrays: every returned topic bit-equal after every callback."""
import numpy as np
import pytest
import torch

import disparity_to_point_cloud_amd as d2pc
import oracle
import colorize_ref as ref
from test_colorize_cpu import node_inputs, structured

pytestmark = pytest.mark.gpu

CALLS = {"D1": "disparity_1", "D2": "disparity_2", "S1": "matching_score_1", "S2": "matching_score_2"}


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q()) as c:
        yield c


def _frames(seed, rows, cols, k=1):
    """{callback: list of k frames}: random disparities, dim blocky scores (see test_colorize_cpu.node_inputs)."""
    rng = np.random.default_rng(seed)
    out = {"D1": [], "D2": [], "S1": [], "S2": []}
    for _ in range(k):
        out["D1"].append(rng.integers(0, 256, size=(rows, cols)).astype(np.uint8))
        out["D2"].append(rng.integers(0, 256, size=(rows, cols)).astype(np.uint8))
        out["S1"].append((structured(rng, rows, cols) // 3).astype(np.uint8))
        out["S2"].append((structured(rng, rows, cols) // 3).astype(np.uint8))
    return out


def _step(node, model, call, frame, what=""):
    got = getattr(node, CALLS[call])(torch.from_numpy(frame).cuda())
    torch.cuda.synchronize()
    want = getattr(model, CALLS[call])(frame)
    assert got.keys() == want.keys(), (what, call, sorted(got), sorted(want))
    for topic, w in want.items():
        g = got[topic].cpu().numpy()
        assert g.shape == w.shape, (what, call, topic, g.shape, w.shape)
        assert np.array_equal(g, w), (what, call, topic, int((g != w).sum()))
    return got, want


def _run(ctx, cols, rows, ox, oy, order, seed=1, **kw):
    node = d2pc.FusionNode(ctx, cols, rows, ox, oy, **kw)
    model = ref.RefNode(cols, rows, ox, oy, rule=kw.get("rule", oracle.FUSE_GRAD_FILTER), form=kw.get("form", 4))
    fr = _frames(seed, rows, cols, k=len(order))
    outs = []
    for i, call in enumerate(order):
        outs.append(_step(node, model, call, fr[call][i], (cols, rows, ox, oy, i)))
    return node, model, outs


def test_reference_geometry(ctx):
    node, model, outs = _run(ctx, 752, 480, -7, 15, ["D1", "S1", "S2", "D2"])
    assert node.n == 465 and node.sq1 == model.sq1 and node.sq2 == model.sq2
    got = outs[-1][0]
    assert tuple(got["cropped_depth_2"].shape) == (465, 465, 3) and tuple(got["combined_score"].shape) == (465, 465)
    assert tuple(got["gradient"].shape) == (425, 425, 3) and tuple(got["fused_depth_map"].shape) == (425, 425)
    assert (got["fused_depth_map"] > 0).any()


@pytest.mark.parametrize("cols,rows,ox,oy", [(188, 120, 0, 0), (120, 188, 3, -5), (160, 160, -4, 9)])
def test_zero_offsets_portrait_and_square(ctx, cols, rows, ox, oy):
    _run(ctx, cols, rows, ox, oy, ["S1", "D1", "S2", "D2"], seed=cols + oy)  # ... and the order S1 D1 S2 D2


def test_camera_2_negated_offsets_and_member_offset_y(ctx):
    """(a): camera 2's square is cropToSquare(rotated, -offset_x, -offset_y) with the side from the member offset_y."""
    node = d2pc.FusionNode(ctx, 752, 480, -7, 15)
    assert node.sq1 == oracle.crop_to_square(752, 480, -7, 15)
    assert node.sq2 == oracle.crop_to_square(480, 752, 7, -15, 15)
    assert node.sq2 != oracle.crop_to_square(480, 752, -7, 15, 15)
    _run(ctx, 200, 140, 6, -9, ["D2", "D1", "S2", "S1", "D2"], seed=3)


def test_fusion_withheld_until_the_fourth_plane(ctx):
    node, model, outs = _run(ctx, 188, 120, -2, 4, ["D2", "S1", "D2", "D1", "D2", "S2", "D2"], seed=4)
    keys = [sorted(o[0]) for o in outs]
    assert keys[0] == keys[2] == keys[4] == ["cropped_depth_2"]
    assert keys[6] == ["combined_score", "cropped_depth_2", "fused_depth_map", "gradient"]


def test_second_fusion_sees_the_overwritten_score(ctx):
    """(b), (c), (d): D1 S1 S2 D2 D2 on the inputs test_colorize_cpu checks to be sensitive; then S1 restores."""
    disp, score = node_inputs()
    node = d2pc.FusionNode(ctx, 188, 120, -2, 4)
    model = ref.RefNode(188, 120, -2, 4)
    _step(node, model, "D1", disp[0])
    _step(node, model, "S1", score[0])
    _step(node, model, "S2", score[1])
    first, wfirst = _step(node, model, "D2", disp[1])
    first_fused = first["fused_depth_map"].cpu().numpy().copy()
    second, wsecond = _step(node, model, "D2", disp[1])
    assert (second["fused_depth_map"].cpu().numpy() != first_fused).any()
    assert (wsecond["fused_depth_map"] != wfirst["fused_depth_map"]).any()
    # no copy: the combined plane IS camera 1's score plane now
    assert second["combined_score"].data_ptr() == node._score1.data_ptr()
    _step(node, model, "S1", score[0])  # S1 between two D2 restores camera 1's score
    third, _ = _step(node, model, "D2", disp[1])
    assert np.array_equal(third["fused_depth_map"].cpu().numpy(), first_fused)


def test_twenty_interleaved_callbacks(ctx):
    rng = np.random.default_rng(20)
    order = [["D1", "D2", "S1", "S2"][i] for i in rng.integers(0, 4, size=20)]
    assert len(set(order)) == 4
    _run(ctx, 170, 130, 3, 5, order, seed=21)


def test_form_cv3_and_another_rule(ctx):
    _run(ctx, 188, 120, -2, 4, ["D1", "S1", "S2", "D2", "D2"], seed=5, form=d2pc.SCORE_FORM_CV3)
    _run(ctx, 188, 120, -2, 4, ["D1", "S1", "S2", "D2"], seed=6, rule=d2pc.FUSE_BETTER_SCORE)


def test_batch_of_three_equals_three_sessions(ctx):
    cols, rows, ox, oy = 188, 120, -2, 4
    order = ["D1", "S1", "S2", "D2", "D2", "S1", "D2"]
    fr = [_frames(30 + k, rows, cols, k=len(order)) for k in range(3)]
    batch = d2pc.FusionNode(ctx, cols, rows, ox, oy, batch=3)
    single = [d2pc.FusionNode(ctx, cols, rows, ox, oy) for _ in range(3)]
    models = [ref.RefNode(cols, rows, ox, oy) for _ in range(3)]
    for i, call in enumerate(order):
        stack = torch.from_numpy(np.stack([fr[k][call][i] for k in range(3)])).cuda()
        got = getattr(batch, CALLS[call])(stack)
        torch.cuda.synchronize()
        for k in range(3):
            one = getattr(single[k], CALLS[call])(stack[k])
            want = getattr(models[k], CALLS[call])(fr[k][call][i])
            torch.cuda.synchronize()
            assert got.keys() == one.keys() == want.keys()
            for topic in want:
                assert torch.equal(got[topic][k], one[topic]), (i, call, k, topic)
                assert np.array_equal(got[topic][k].cpu().numpy(), want[topic]), (i, call, k, topic)


def test_captured_disparity_2_replays_on_new_frames(ctx):
    """matching_score_1 + disparity_2 captured as one graph (four launches in a row on the capture stream: no
    parallel branches) and replayed on new frame contents, against an eager session and the model.  The score
    planes' swap is host state, so a capture is pinned to the planes of its capture: the pair S1, D2 is the unit
    that replays like the eager node (FusionNode's docstring)."""
    cols, rows, ox, oy = 752, 480, -7, 15
    fr = _frames(40, rows, cols, k=4)
    node, eager = (d2pc.FusionNode(ctx, cols, rows, ox, oy) for _ in range(2))
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


def test_wrong_frames_raise_value_error(ctx):
    node = d2pc.FusionNode(ctx, 188, 120)
    ok = torch.zeros((120, 188), dtype=torch.uint8, device="cuda")
    node.disparity_1(ok)
    for call in CALLS.values():
        fn = getattr(node, call)
        with pytest.raises(ValueError):
            fn(torch.zeros((188, 120), dtype=torch.uint8, device="cuda"))       # shape
        with pytest.raises(ValueError):
            fn(torch.zeros((120, 188), dtype=torch.int16, device="cuda"))       # dtype (mono16 is out of scope)
        with pytest.raises(ValueError):
            fn(torch.zeros((120, 188), dtype=torch.uint8))                      # host tensor
        with pytest.raises(ValueError):
            fn(np.zeros((120, 188), dtype=np.uint8))                            # not a tensor
        with pytest.raises(ValueError):
            fn(torch.zeros((120, 376), dtype=torch.uint8, device="cuda")[:, ::2])  # column stride 2
    b3 = d2pc.FusionNode(ctx, 188, 120, batch=3)
    with pytest.raises(ValueError):
        b3.disparity_1(ok)
    with pytest.raises(ValueError):
        d2pc.FusionNode(ctx, 188, 120, batch=0)
