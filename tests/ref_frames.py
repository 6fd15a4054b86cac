"""Input frames and callback scripts of the reference-pinned fusion tests (tests/golden/reference_fusion.npz).

Frames come from a 32-bit linear congruential generator written out here, so that no library's random stream has to
stay what it is today:  x <- (1664525 x + 1013904223) mod 2^32  (Numerical Recipes' constants), one step per pixel in
row-major order, the pixel taken from the top bits.  lcg_words() evaluates the recurrence by doubling
(x[k+m] = A[k] x[m] + C[k]), which is the same sequence as the scalar loop (test_reference_cpu checks it).

  depth frames   x >> 24: every byte value, no structure
  score frames   a tiling of flat patches (levels 0, 45, 90, 135, 180) + x >> 28: edges in both directions, so the
                 score filter's threshold fires in places and stays silent in others
"""
import hashlib
import json
import os

import numpy as np

LCG_A, LCG_C = 1664525, 1013904223
MASK = 0xFFFFFFFF

CALL_NAMES = ("D1", "D2", "S1", "S2")
# the reference's publishing order inside one callback (src/depth_map_fusion.cpp:59, :126, :132, :136)
TOPIC_ORDER = ("cropped_depth_1", "cropped_depth_2", "cropped_score_1", "cropped_score_2", "combined_score", "gradient",
               "fused_depth_map")


def lcg_words(seed, count):
    """x[1..count] of the recurrence started at x[0] = seed, as uint32."""
    a = np.array([1], dtype=np.uint64)   # x[k] = a[k] x[0] + c[k]
    c = np.array([0], dtype=np.uint64)
    while a.size < count + 1:
        am = (int(a[-1]) * LCG_A) & MASK
        cm = (int(c[-1]) * LCG_A + LCG_C) & MASK
        a, c = np.concatenate([a, (a * np.uint64(am)) & np.uint64(MASK)]), np.concatenate([c, (a * np.uint64(cm) + c) & np.uint64(MASK)])
    x = (a[1:count + 1] * np.uint64(seed & MASK) + c[1:count + 1]) & np.uint64(MASK)
    return x.astype(np.uint32)


def lcg_words_scalar(seed, count):
    """The recurrence as written, one step at a time (the check of lcg_words)."""
    out, x = [], seed & MASK
    for _ in range(count):
        x = (LCG_A * x + LCG_C) & MASK
        out.append(x)
    return np.array(out, dtype=np.uint32)


def frame(seed, call, rows, cols):
    """The frame of callback `call` ("D1", "D2", "S1", "S2"): uint8 (rows, cols)."""
    w = lcg_words(seed, rows * cols).reshape(rows, cols)
    if call[0] == "D":
        return (w >> np.uint32(24)).astype(np.uint8)
    r, c = np.arange(rows)[:, None], np.arange(cols)[None, :]
    level = ((r // 9 + 2 * (c // 7) + seed) % 5) * 45
    return (level + (w >> np.uint32(28))).astype(np.uint8)


def frame_seed(script_seed, index):
    return (script_seed * 1000003 + 7919 * index + 1) & MASK


# name: (cols, rows, offset_x, offset_y, score form, seed, callbacks, stored in full?)
# 75 x 58 with (-2, 5): n = 53, a 13 x 13 fused map; its rotated portrait twin; the same in the OpenCV 3 score form.
# 200 x 140 with (-6, 9): n = 131 -- three tile columns of k_node_fuse, a ragged last tile, the crop across a tile seam.
# 752 x 480 with (-7, 15): the reference's launch file.
SCRIPTS = {
    "small_landscape": (75, 58, -2, 5, 4, 11, ("D2", "S1", "D1", "S2", "D2", "D2", "S1", "D2"), True),
    "small_portrait": (58, 75, -2, 5, 4, 12, ("S2", "D1", "S1", "D2", "S1", "D2", "D2"), True),
    "small_landscape_cv3": (75, 58, -2, 5, 3, 13, ("S1", "S2", "D1", "D2", "D2"), True),
    "tiles_200x140": (200, 140, -6, 9, 4, 14, ("S1", "S2", "D1", "D2", "D2", "S1", "D2", "D1", "S2", "D2"), False),
    "launch_752x480": (752, 480, -7, 15, 4, 15, ("D1", "D2", "S1", "S2", "D2", "D2", "S1", "D2"), False),
}


def script_frames(name):
    cols, rows, _, _, _, seed, calls, _ = SCRIPTS[name]
    return [frame(frame_seed(seed, i), call, rows, cols) for i, call in enumerate(calls)]


def digest(data) -> str:
    return hashlib.sha256(bytes(data)).hexdigest()


def topic_array(encoding, width, height, data):
    a = np.frombuffer(data, dtype=np.uint8)
    return a.reshape(height, width, 3) if encoding == "rgb8" else a.reshape(height, width)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fusion.npz")


def load_golden(path=GOLDEN):
    """tests/golden/reference_fusion.npz (make_reference_golden.py) -> (index dict, {key: array})."""
    z = np.load(path)
    arrays = {k: z[k] for k in z.files}
    return json.loads(arrays["index"].tobytes().decode()), arrays
