"""The depth_map_fusion node on the device against recorded runs of the COMPILED reference
(tests/golden/reference_fusion.npz, written by tests/golden/make_reference_golden.py from the reference's unmodified
depth_map_fusion.cpp; test_reference_cpu.py keeps the file equal to what the reference gives).  Reads that file and
tests/ref_frames.py only: the checker here is the reference's own output, not a model this project wrote.

Every script is replayed, callback by callback, through FusionSession with the single-launch fusing callback, FusionSession
with the three-launch composition, the Python FusionNode and the host mirror (host/depth_map_fusion_amd.hpp via
`d2pc_replay fusion`).  After every callback the published topics are the recorded ones -- for the host mirror in the
recorded order too -- with the recorded sizes, encodings and bytes (the small scripts store the bytes, the larger
ones their SHA-256).

Also here: the refusal of |offset_x| > |offset_y| on the surfaces that need a device (d2pc_fusion_node_create's error
text, the host mirror's dropped frame)."""
import os
import subprocess

import numpy as np
import pytest
import torch

import disparity_to_point_cloud_amd as d2pc

import ref_frames

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPLAY = os.path.join(ROOT, "host", "d2pc_replay")
CALLS = {"D1": "disparity_1", "D2": "disparity_2", "S1": "matching_score_1", "S2": "matching_score_2"}


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q()) as c:
        yield c


@pytest.fixture(scope="module")
def golden():
    index, arrays = ref_frames.load_golden()
    assert sorted(index) == sorted(ref_frames.SCRIPTS)
    return index, arrays


def _frames(golden, name):
    """The script's input frames: regenerated, and equal to the stored ones where the file stores them."""
    index, arrays = golden
    frames = ref_frames.script_frames(name)
    if index[name]["stored"]:
        for i, f in enumerate(frames):
            assert np.array_equal(f, arrays["%s/in/%d" % (name, i)]), (name, i)
    return frames


def _check_topic(golden, name, i, record, data, width, height, channels, who):
    """One published image against its record [topic, encoding, width, height, step, sha256]."""
    index, arrays = golden
    topic, enc, w, h, step, sha = record
    assert (width, height, channels) == (w, h, 3 if enc == "rgb8" else 1), (who, name, i, topic, (width, height, channels), (w, h, enc))
    assert step == w * channels
    data = bytes(data)
    assert len(data) == step * h, (who, name, i, topic)
    if index[name]["stored"]:
        want = arrays["%s/out/%d/%s" % (name, i, topic)]
        got = np.frombuffer(data, dtype=np.uint8).reshape(want.shape)
        assert np.array_equal(got, want), (who, name, i, topic, int((got != want).sum()), "bytes differ")
    assert ref_frames.digest(data) == sha, (who, name, i, topic)


@pytest.mark.parametrize("who", ["single_launch", "three_launches", "FusionNode"])
@pytest.mark.parametrize("name", list(ref_frames.SCRIPTS))
def test_device_sessions_replay_the_reference(ctx, golden, name, who):
    e = golden[0][name]
    cols, rows, ox, oy, form = e["cols"], e["rows"], e["offset_x"], e["offset_y"], e["form"]
    if who == "FusionNode":
        node = d2pc.FusionNode(ctx, cols, rows, ox, oy, form=form)
    else:
        node = d2pc.FusionSession(ctx, cols, rows, ox, oy, form=form, single_launch=int(who == "single_launch"))
        assert node.cfg.single_launch == int(who == "single_launch")
    for i, (call, f) in enumerate(zip(e["calls"], _frames(golden, name))):
        got = getattr(node, CALLS[call])(torch.from_numpy(f).cuda())
        torch.cuda.synchronize()
        records = e["published"][i]
        assert sorted(got) == sorted(r[0] for r in records), (who, name, i, call)
        for r in records:
            a = got[r[0]].cpu().numpy()
            _check_topic(golden, name, i, r, a.tobytes(), a.shape[1], a.shape[0], a.shape[2] if a.ndim == 3 else 1, who)
    if who != "FusionNode":
        node.close()


def _replay(tmp_path, steps, cols, rows, *extra):
    """steps: [(callback, frame)] -> (index rows, payloads, dropped, stderr) of `d2pc_replay fusion`."""
    assert os.path.exists(REPLAY), "host/d2pc_replay is not built"
    lines = []
    for i, (call, f) in enumerate(steps):
        (tmp_path / f"f{i}.raw").write_bytes(np.ascontiguousarray(f).tobytes())
        lines.append(f"{call} f{i}.raw")
    (tmp_path / "script.txt").write_text("\n".join(lines) + "\n")
    prefix = str(tmp_path / "out")
    p = subprocess.run([REPLAY, "fusion", str(tmp_path / "script.txt"), str(cols), str(rows), "mono8", prefix] + list(extra),
                       capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stderr[-2000:])
    index = open(prefix + ".index").read().splitlines()
    assert index[-1].startswith("dropped ")
    rows_ = [ln.split() for ln in index[:-1]]
    payloads = [open(f"{prefix}.{i}.raw", "rb").read() for i in range(len(rows_))]
    return rows_, payloads, int(index[-1].split()[1]), p.stderr


# d2pc_replay has no switch for the score form: the host mirror runs the library's default, OpenCV 4's
@pytest.mark.parametrize("name", [n for n, s in ref_frames.SCRIPTS.items() if s[4] == 4])
def test_host_mirror_replays_the_reference_in_its_order(ctx, golden, tmp_path, name):
    e = golden[0][name]
    cols, rows = e["cols"], e["rows"]
    steps = list(zip(e["calls"], _frames(golden, name)))
    got, payloads, dropped, _ = _replay(tmp_path, steps, cols, rows, f"offset_x={e['offset_x']}", f"offset_y={e['offset_y']}")
    assert dropped == 0
    k = 0
    for i, records in enumerate(e["published"]):
        for r in records:                       # the reference's publishing order
            num, at, topic, width, height, enc, step, frame_id, stamp, nbytes = got[k]
            assert (int(num), int(at), topic, enc, int(step)) == (k, i + 1, "/" + r[0], r[1], r[4]), (name, i, got[k], r)
            assert int(nbytes) == len(payloads[k])
            _check_topic(golden, name, i, r, payloads[k], int(width), int(height), 3 if enc == "rgb8" else 1, "host mirror")
            k += 1
    assert k == len(got)


def test_offset_x_beyond_offset_y_is_refused_on_the_device_surfaces(ctx, tmp_path):
    """d2pc_fusion_node_create: D2PC_ERR_BAD_SIZE and a last-error text that names both offsets; FusionNode the same
    status; the host mirror drops every frame with its usual warning and publishes nothing."""
    cols, rows, ox, oy = 200, 140, 9, -6
    with pytest.raises(d2pc.D2pcError) as e:
        d2pc.FusionSession(ctx, cols, rows, ox, oy)
    assert e.value.status == 3
    text = str(e.value)            # carries d2pc_last_error
    assert "offset_x" in text and "offset_y" in text and "(9)" in text and "(-6)" in text, text
    with pytest.raises(d2pc.D2pcError) as e:
        d2pc.FusionNode(ctx, cols, rows, ox, oy)
    assert e.value.status == 3
    steps = [(c, ref_frames.frame(7 + i, c, rows, cols)) for i, c in enumerate(["S1", "D1", "S2", "D2"])]
    got, payloads, dropped, err = _replay(tmp_path, steps, cols, rows, f"offset_x={ox}", f"offset_y={oy}")
    assert dropped == 4 and got == [] and err.count("frame dropped") == 4 and "offset_x" in err
    # the same frames with the magnitudes swapped are served
    got, payloads, dropped, err = _replay(tmp_path, steps, cols, rows, f"offset_x={oy}", f"offset_y={ox}")
    assert dropped == 0 and [r[2] for r in got][-1] == "/fused_depth_map" and (int(got[-1][3]), int(got[-1][4])) == (91, 91)
