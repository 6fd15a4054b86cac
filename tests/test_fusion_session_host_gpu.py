"""The host side of the depth_map_fusion session: d2pc_fusion_node_callback (frames and topics in host memory) and the
C++ mirror of the reference class (host/depth_map_fusion_amd.hpp) through `d2pc_replay fusion`, against
colorize_ref.RefNode -- every topic's bytes, size, encoding, step and header."""
import os
import subprocess

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import colorize_ref as ref
from test_colorize_cpu import structured

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "host", "d2pc_replay")
WHICH = {"D1": d2pc.NODE_DISPARITY_1, "D2": d2pc.NODE_DISPARITY_2, "S1": d2pc.NODE_MATCHING_SCORE_1,
         "S2": d2pc.NODE_MATCHING_SCORE_2}
MODEL = {"D1": "disparity_1", "D2": "disparity_2", "S1": "matching_score_1", "S2": "matching_score_2"}
# the reference's publishing order inside one callback (:59, :126, :132, :136)
ORDER = ["cropped_depth_1", "cropped_depth_2", "cropped_score_1", "cropped_score_2", "combined_score", "gradient",
         "fused_depth_map"]


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q()) as c:
        yield c


def _frame(rng, call, rows, cols):
    if call[0] == "D":
        return rng.integers(0, 256, size=(rows, cols)).astype(np.uint8)
    return (structured(rng, rows, cols) // 3).astype(np.uint8)


@pytest.mark.parametrize("single", [1, 0])
def test_host_entry_equals_the_model(ctx, single):
    cols, rows, ox, oy = 188, 120, -2, 4
    s = d2pc.FusionSession(ctx, cols, rows, ox, oy, single_launch=single)
    model = ref.RefNode(cols, rows, ox, oy)
    rng = np.random.default_rng(90)
    for i, call in enumerate(["D2", "D1", "S1", "S2", "D2", "D2", "S1", "D2", "S2", "D1", "D2"]):
        f = _frame(rng, call, rows, cols)
        if i % 3 == 1:  # rows further apart than the width
            wide = np.zeros((rows, cols + 13), dtype=np.uint8)
            wide[:, :cols] = f
            f = wide[:, :cols]
            assert f.strides == (cols + 13, 1)
        got = s.callback_host(WHICH[call], f)
        want = getattr(model, MODEL[call])(np.ascontiguousarray(f))
        assert got.keys() == want.keys(), (i, call)
        for topic, w in want.items():
            assert got[topic].shape == w.shape and np.array_equal(got[topic], w), (i, call, topic)
    s.close()


def test_host_entry_batch(ctx):
    cols, rows, ox, oy = 120, 150, 2, -3
    s = d2pc.FusionSession(ctx, cols, rows, ox, oy, batch=3)
    models = [ref.RefNode(cols, rows, ox, oy) for _ in range(3)]
    rng = np.random.default_rng(91)
    for call in ["D1", "S1", "S2", "D2", "D2"]:
        fr = np.stack([_frame(rng, call, rows, cols) for _ in range(3)])
        got = s.callback_host(WHICH[call], fr)
        for k in range(3):
            for topic, w in getattr(models[k], MODEL[call])(fr[k]).items():
                assert np.array_equal(got[topic][k], w), (call, k, topic)
    s.close()


def test_too_small_topic_buffer_gives_capacity_and_the_node_lives_on(ctx):
    cols, rows, ox, oy = 188, 120, -2, 4
    s = d2pc.FusionSession(ctx, cols, rows, ox, oy)
    model = ref.RefNode(cols, rows, ox, oy)
    rng = np.random.default_rng(92)
    fr = {c: _frame(rng, c, rows, cols) for c in ("D1", "S1", "S2", "D2")}
    n = s.n
    with pytest.raises(d2pc.D2pcError) as e:
        s.callback_host(WHICH["D1"], fr["D1"], capacity={"cropped_depth_1": 3 * n * n - 1})
    assert e.value.status == 4
    for c in ("D1", "S1", "S2"):
        s.callback_host(WHICH[c], fr[c]), getattr(model, MODEL[c])(fr[c])
    # refused BEFORE anything ran: the fusion that follows is the node's FIRST (the score plane has not been fused over)
    for topic in ("gradient", "fused_depth_map", "combined_score", "cropped_depth_2"):
        with pytest.raises(d2pc.D2pcError) as e:
            s.callback_host(WHICH["D2"], fr["D2"], capacity={topic: 10})
        assert e.value.status == 4, topic
    # a short buffer for a topic this callback does not publish is no error
    got = s.callback_host(WHICH["D2"], fr["D2"], capacity={"cropped_depth_1": 0, "cropped_score_2": 1})
    want = model.disparity_2(fr["D2"])
    assert got.keys() == want.keys()
    for topic, w in want.items():
        assert np.array_equal(got[topic], w), topic
    s.close()


def _replay(tmp_path, steps, cols, rows, *extra):
    """steps: [(callback, frame)] -> (index rows, payloads, dropped) of `d2pc_replay fusion`."""
    assert os.path.exists(REPLAY), "host/d2pc_replay is not built"
    lines = ["# a replayed camera rig"]
    for i, (call, f) in enumerate(steps):
        (tmp_path / f"f{i}.raw").write_bytes(np.ascontiguousarray(f).tobytes())
        size = "" if f.shape == (rows, cols) else f" {f.shape[1]} {f.shape[0]}"
        lines.append(f"{call} f{i}.raw{size}")
    (tmp_path / "script.txt").write_text("\n".join(lines) + "\n")
    prefix = str(tmp_path / "out")
    p = subprocess.run([REPLAY, "fusion", str(tmp_path / "script.txt"), str(cols), str(rows), "mono8", prefix] + list(extra),
                       capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    index = open(prefix + ".index").read().splitlines()
    assert index[-1].startswith("dropped ")
    rows_ = [ln.split() for ln in index[:-1]]
    payloads = [open(f"{prefix}.{i}.raw", "rb").read() for i in range(len(rows_))]
    return rows_, payloads, int(index[-1].split()[1]), p.stderr


@pytest.mark.parametrize("extra", [(), ("single_launch=0",)])
def test_replay_reproduces_the_model_topics_headers_and_encodings(ctx, tmp_path, extra):
    cols, rows, ox, oy = 752, 480, -7, 15
    rng = np.random.default_rng(93)
    order = ["D1", "D2", "S1", "S2", "D2", "D2", "S1", "D2"]
    steps = [(c, _frame(rng, c, rows, cols)) for c in order]
    got, payloads, dropped, _ = _replay(tmp_path, steps, cols, rows, f"offset_x={ox}", f"offset_y={oy}", *extra)
    assert dropped == 0
    model = ref.RefNode(cols, rows, ox, oy)
    k = 0
    for i, (call, f) in enumerate(steps):
        want = getattr(model, MODEL[call])(f)
        line = i + 2  # the script's first line is a comment
        for topic in [t for t in ORDER if t in want]:
            w = want[topic]
            num, at, name, width, height, enc, step, frame_id, stamp, nbytes = got[k]
            ch = 3 if w.ndim == 3 else 1
            assert (int(num), int(at), name) == (k, line, "/" + topic), (i, call, topic, got[k])
            assert (int(width), int(height), enc, int(step)) == (w.shape[1], w.shape[0], "rgb8" if ch == 3 else "mono8", w.shape[1] * ch)
            assert (frame_id, stamp) == (f"cam_{call}", f"{1000 + line}.{7 * line}")   # the incoming message's header
            assert int(nbytes) == w.size and payloads[k] == w.tobytes(), (i, call, topic)
            k += 1
    assert k == len(got) == 1 + 1 + 1 + 1 + 4 + 4 + 1 + 4


def test_replay_missing_params_warn_and_default_to_zero(ctx, tmp_path):
    cols, rows = 188, 120
    rng = np.random.default_rng(94)
    steps = [(c, _frame(rng, c, rows, cols)) for c in ["S1", "D1", "S2", "D2"]]
    got, payloads, dropped, err = _replay(tmp_path, steps, cols, rows)
    assert "Failed to load parameter offset_x" in err and "Failed to load parameter offset_y" in err   # :119-124
    model = ref.RefNode(cols, rows, 0, 0)
    want = {}
    for call, f in steps:
        want = getattr(model, MODEL[call])(f)
    assert dropped == 0 and len(got) == 7
    assert payloads[-1] == want["fused_depth_map"].tobytes() and got[-1][2] == "/fused_depth_map"


def test_replay_drops_a_frame_of_another_size_and_lives_on(ctx, tmp_path):
    cols, rows, ox, oy = 188, 120, -2, 4
    rng = np.random.default_rng(95)
    good = [(c, _frame(rng, c, rows, cols)) for c in ["D1", "S1", "S2"]]
    stray = ("D1", rng.integers(0, 256, size=(rows + 8, cols - 4)).astype(np.uint8))
    last = ("D2", _frame(rng, "D2", rows, cols))
    got, payloads, dropped, err = _replay(tmp_path, good + [stray, last], cols, rows, f"offset_x={ox}", f"offset_y={oy}")
    assert dropped == 1 and "frame dropped" in err
    model = ref.RefNode(cols, rows, ox, oy)
    for call, f in good:
        getattr(model, MODEL[call])(f)
    want = model.disparity_2(last[1])   # camera 1's depth is still the one of the good D1
    assert [r[2] for r in got] == ["/cropped_depth_1", "/cropped_score_1", "/cropped_score_2", "/cropped_depth_2",
                                   "/combined_score", "/gradient", "/fused_depth_map"]
    for r, p in zip(got[3:], payloads[3:]):
        assert p == want[r[2][1:]].tobytes(), r[2]
