"""Where the data lies: memory layouts for the device entry points of include/d2pc.h, as data (no GPU, no allocation).

Every other pattern module of this suite varies the VALUES a kernel sees; this one varies the ADDRESSES.  A layout
places `n_frames` frames of `rows` rows of `row_bytes` bytes inside an arena of `arena_bytes` bytes: the plane's pointer
is the arena's base plus `base`, rows are `pitch` bytes apart, frames `frame_stride` bytes apart.  The byte a kernel
means by (frame f, row r, column byte c) is

    base + f * frame_stride + r * pitch + c                                    (all of it in 64 bits)

and `touched(layout, slip)` restates that sum with one slip at a time, the way a kernel would get it wrong:

    frame32   f * frame_stride taken modulo 2^32 (a 32-bit product, or a stride field narrowed to 32 bits)
    row32     r * pitch taken modulo 2^32 (a product of two 32-bit operands cast afterwards)
    row_i32   the same, then sign-extended (an `int` offset)
    sum32     the whole offset from the plane's pointer taken modulo 2^32

The model works on row starts: a row that contains offset 2^32 itself counts as unslipped under sum32 (its start is
below), which only makes the kill matrix harder to fill.  tests/test_address_patterns.py asserts what every layout was
built to reach, that every slip which applies to it moves at least one row, that every slipped byte stays inside the
arena (a kernel with that slip FAILS the comparison of tests/test_address_range_gpu.py, it does not fault) and that no
slipped frame coincides with another frame's true place.
"""
from collections import namedtuple

import numpy as np

G = 1 << 32
H = 1 << 31
SENTINEL = 0xA5
SLIPS = ("frame32", "row32", "row_i32", "sum32")
# which slips a layout is built to kill ("far" covers both of its variants); everything else is left to the other layouts
APPLIES = {
    "dense": (),
    "far": ("frame32", "sum32"),
    "straddle": ("sum32",),
    "tall": ("row32", "row_i32", "sum32"),
    "high": ("row_i32",),
}
KINDS = ("dense", "far16", "far1", "straddle", "tall", "high")

Layout = namedtuple("Layout", "name arena_bytes base pitch frame_stride rows row_bytes n_frames")


def family(layout_or_name):
    name = layout_or_name if isinstance(layout_or_name, str) else layout_or_name.name
    return "far" if name.startswith("far") else name


def frame_extent(L):
    """Plane::frame_extent of d2pc_plane.hpp: a frame ends with the last byte of its last row."""
    return (L.rows - 1) * L.pitch + L.row_bytes


def extent(L):
    return (L.n_frames - 1) * L.frame_stride + frame_extent(L)


def _up(x, a):
    return (x + a - 1) // a * a


def _arena(base, ext):
    return _up(base + ext + 256, 4096)


def dense(rows, row_bytes, n_frames=2, pad=0, base=0):
    """Contiguous frames (rows `pad` bytes longer than their pixels): the baseline."""
    pitch = row_bytes + pad
    L = Layout("dense", 0, base, pitch, rows * pitch, rows, row_bytes, n_frames)
    return L._replace(arena_bytes=_arena(base, extent(L)))


def far(rows, row_bytes, elem=1, aligned=True, n_frames=2):
    """Frames 2^32 + a little apart.  aligned: pointer, pitch and stride are multiples of 16, so that 16-byte row loads
    run ("far16"); otherwise all three are off by one element ("far1": the scalar paths).  The little is 4096 (+ elem):
    a stride cut to 32 bits puts frame 1 on top of frame 0, shifted."""
    if aligned:
        pitch, base, stride = _up(row_bytes, 16), 256, G + 4096
    else:
        pitch, base, stride = _up(row_bytes, 16) + elem, 256 + elem, G + 4096 + elem
    L = Layout("far16" if aligned else "far1", 0, base, pitch, stride, rows, row_bytes, n_frames)
    return L._replace(arena_bytes=_arena(base, extent(L)))


def straddle(rows, row_bytes, elem=1, align=None, n_frames=2):
    """Two frames 2^32 - extent / 2 apart (rounded down to the alignment): offset 2^32 from the plane's pointer falls
    inside frame 1."""
    align = align or max(elem, 16)
    pitch = _up(row_bytes, 16)
    L = Layout("straddle", 0, 256, pitch, 0, rows, row_bytes, n_frames)
    L = L._replace(frame_stride=(G - frame_extent(L) // 2) // align * align)
    return L._replace(arena_bytes=_arena(L.base, extent(L)))


def tall(rows, row_bytes, elem=1):
    """ONE frame with a pitch of 2^26 + 33 (+ 34 for 16-bit rows: a multiple of the element) and at least 66 rows, so
    that rows 64.. start above 2^32 and row 63 one pitch below it; the plane's pointer sits 2^31 into the arena, so that
    a sign-extended row offset (rows 32..63) stays inside the allocation."""
    assert rows >= 66
    pitch = (1 << 26) + (33 if elem == 1 else 34)
    L = Layout("tall", 0, H, pitch, 0, rows, row_bytes, 1)
    return L._replace(arena_bytes=_arena(H, extent(L)))


def high(rows, row_bytes, pitch=None):
    """ONE frame on the host limit of the entry points that form in-frame offsets in 32 bits: the largest pitch with
    rows * pitch <= 2^32 - 1 (Bound32::Plane), or the pitch handed in (d2pc_process_device, whose rule is make_geom's).
    The pointer sits 2^31 into the arena: an `int` offset (the rows above 2^31) lands on bytes of the same allocation."""
    pitch = pitch or plane_max_pitch(rows)
    L = Layout("high", 0, H, pitch, 0, rows, row_bytes, 1)
    return L._replace(arena_bytes=_arena(H, extent(L)))


def make(kind, rows, row_bytes, elem=1, n_frames=2, pitch=None):
    if kind == "dense":
        return dense(rows, row_bytes, n_frames)
    if kind in ("far16", "far1"):
        return far(rows, row_bytes, elem, kind == "far16", n_frames)
    if kind == "straddle":
        return straddle(rows, row_bytes, elem, n_frames=n_frames)
    if kind == "tall":
        return tall(rows, row_bytes, elem)
    if kind == "high":
        return high(rows, row_bytes, pitch)
    raise KeyError(kind)


# ------------------------------------------------------------------------------------------ the hosts' rules, restated
def plane_fits(pitch, frame_stride, rows, row_bytes, n_frames, bound, whole_rows=False):
    """Plane::fits (d2pc_plane.hpp).  bound: "plane" (pitch * rows <= 2^32 - 1) or "pitch" (pitch <= 2^32 - 1)."""
    if pitch < row_bytes:
        return False
    if (pitch * rows if bound == "plane" else pitch) > 0xFFFFFFFF:
        return False
    return n_frames <= 1 or frame_stride >= (rows * pitch if whole_rows else (rows - 1) * pitch + row_bytes)


def plane_max_pitch(rows):
    return 0xFFFFFFFF // rows


def geom_fits(width, height, row_stride, in_frame_stride, n_frames, elem):
    """The layout rules of make_geom (d2pc_capi_route.hip), the ROI / tile-count rules left out."""
    if width <= 0 or height <= 0 or width * height > (1 << 31):
        return False
    if row_stride < width * elem or row_stride % elem:
        return False
    if n_frames > 1 and (in_frame_stride < height * row_stride or in_frame_stride % elem):
        return False
    return (height + 4097) * row_stride <= 0xFFFFFFFF


# d2pc_process_device on `high`: f32, 96 columns, a 16-column ROI at border 40
HIGH_PROCESS = dict(width=96, height=61440, row_stride=65532, elem=4, border=40)
# Bound32::Plane entry points on `high`
HIGH_PLANE_ROWS = 465

# points are counted in records of 16 bytes (indices: 4): frame 1 of the points lies 2^32 + 256 bytes in
FAR_POINT_STRIDE = (1 << 28) + 16
FAR_INDEX_POINT_STRIDE = (1 << 30) + 16   # ... and frame 1 of the INDEX plane 2^32 + 64 bytes in (points: 16 GiB)


def points(kind, roi_n, n_frames=2, rec=16, base=256, point_stride=None):
    """The output of the reprojection as a layout in bytes: a frame is roi_n packed records (the model's "rows": a
    kernel forms point_index * 16 as it forms row * pitch), frames a whole number of records apart (`point_stride`;
    default: what the kind asks of a 16-byte record)."""
    if point_stride is None:
        if kind == "dense":
            point_stride = roi_n + 5
        elif kind in ("far16", "far1"):
            point_stride = FAR_POINT_STRIDE
        elif kind == "straddle":
            point_stride = (G - roi_n * 16 // 2) // 16 // 8 * 8
        else:
            raise KeyError(kind)
    L = Layout(kind, 0, base, rec, point_stride * rec, roi_n, rec, n_frames)
    return L._replace(arena_bytes=_arena(base, extent(L)))


# ---------------------------------------------------------------------------------------------------- what is touched
def _wrap32(x):
    return x % G


def _sext32(x):
    x = x % G
    return np.where(x >= H, x - G, x)


def row_offsets(L, slip=None):
    """(n_frames, rows) int64: where each row starts, counted from the plane's pointer, with one slip or none."""
    f = np.arange(L.n_frames, dtype=np.int64)[:, None] * np.int64(L.frame_stride)
    r = np.arange(L.rows, dtype=np.int64)[None, :] * np.int64(L.pitch)
    if slip is None:
        return f + r
    if slip == "frame32":
        return _wrap32(f) + r
    if slip == "row32":
        return f + _wrap32(r)
    if slip == "row_i32":
        return f + _sext32(r)
    if slip == "sum32":
        return _wrap32(f + r)
    raise KeyError(slip)


def touched(L, slip=None):
    """(n_frames, rows, 2) int64: [start, end) of every row in ARENA bytes, as a kernel with `slip` would address it."""
    s = row_offsets(L, slip) + np.int64(L.base)
    return np.stack([s, s + np.int64(L.row_bytes)], axis=-1)


def killed(L, slip):
    """Does the slip move a row of this layout?"""
    return not np.array_equal(touched(L, slip), touched(L))


def inside_arena(L, slip=None):
    t = touched(L, slip)
    return bool(t[..., 0].min() >= 0 and t[..., 1].max() <= L.arena_bytes)


def coincides_with_another_frame(L, slip):
    """Does a slipped frame sit exactly where ANOTHER frame truly is?  (It would then read / write valid data of the
    wrong frame -- still a failure, since frames differ in content, but a different one; the layouts avoid it.)"""
    t, s = touched(L), touched(L, slip)
    return any(np.array_equal(s[f], t[g]) for f in range(L.n_frames) for g in range(L.n_frames) if f != g)


# ------------------------------------------------------------------------ the geometries the GPU file uses, by subject
# (subject, rows, row bytes, element bytes, layout kinds): every plane tests/test_address_range_gpu.py lays out
PLANES = [
    ("process_device input 203x131 f32", 131, 812, 4, ("far16", "far1", "straddle")),
    ("process_device input 204x131 f32", 131, 816, 4, ("far16",)),
    ("process_device input 203x131 u8 / median / mono8", 131, 203, 1, ("far16", "far1", "straddle")),
    ("process_device input 204x131 u8", 131, 204, 1, ("far16",)),
    ("process_device input 203x131 u16 / mono16", 131, 406, 2, ("far16", "far1", "straddle")),
    ("process_device input 204x131 u16", 131, 408, 2, ("far16",)),
    ("median / mono8 203x70", 70, 203, 1, ("tall",)),
    ("mono16 203x70", 70, 406, 2, ("tall",)),
    ("rotate / colorize source 129x65", 65, 129, 1, ("far16", "far1", "straddle")),
    ("rotated 65x129", 129, 65, 1, ("far16", "far1", "straddle")),
    ("rotate / colorize 129x70, source or destination", 70, 129, 1, ("tall",)),
    ("colorize gray view 124x62", 62, 124, 1, ("far16", "far1", "straddle")),
    ("colorize rgb view 124x62", 62, 372, 1, ("far16", "far1", "straddle")),
    ("colorize gray view 60x126 (rotated)", 126, 60, 1, ("far16", "far1", "straddle")),
    ("colorize rgb view 60x126 (rotated)", 126, 180, 1, ("far16", "far1", "straddle")),
    ("colorize rgb 129x70", 70, 387, 1, ("tall",)),
    ("fusion 249x9", 9, 249, 1, ("far16", "far1", "straddle")),
    ("fused 241x6", 6, 241, 1, ("far16", "far1", "straddle")),
    ("fusion 61x83", 83, 61, 1, ("far16", "far1", "straddle")),
    ("fused 53x80", 80, 53, 1, ("far16", "far1", "straddle")),
    ("fusion 61x465", HIGH_PLANE_ROWS, 61, 1, ("high",)),
    ("fused 53x462", HIGH_PLANE_ROWS - 3, 53, 1, ("high",)),
    ("score source 58x55", 55, 58, 1, ("far16", "far1", "straddle")),
    ("score source 83x80", 80, 83, 1, ("far16", "far1", "straddle")),
    ("score source 80x465", HIGH_PLANE_ROWS, 80, 1, ("high",)),
    ("score square 45", 45, 45, 1, ("far16", "far1", "straddle", "high")),
    ("score square 70", 70, 70, 1, ("far16", "far1", "straddle", "high")),
    ("node frames 188x120", 120, 188, 1, ("far16", "far1", "straddle")),
    ("node camera 2, 188x70", 70, 188, 1, ("tall",)),
]


def gpu_geometries():
    """(subject, layout) for every layout tests/test_address_range_gpu.py builds: the CPU test walks this list, and the
    GPU test refuses a layout that is not in it."""
    out = [(s, make(k, rows, rb, es, 1 if k in ("tall", "high") else 2)) for s, rows, rb, es, kinds in PLANES for k in kinds]
    hp = HIGH_PROCESS
    out.append(("process_device input high", high(hp["height"], hp["width"] * hp["elem"], hp["row_stride"])))
    for roi_n in (123 * 51, 124 * 51):
        for kind in ("far16", "straddle"):
            out.append(("points of %d" % roi_n, points(kind, roi_n)))
    out.append(("index plane past 4 GiB", points("far16", 123 * 51, rec=4, point_stride=FAR_INDEX_POINT_STRIDE)))
    return out


def kill_matrix():
    """{layout family: {slip: "X" (every geometry of the GPU file is killed), "." (does not apply)}}, and the text."""
    m = {k: {s: "." for s in SLIPS} for k in APPLIES}
    for _, L in gpu_geometries():
        for s in APPLIES[family(L)]:
            m[family(L)][s] = "X" if killed(L, s) and m[family(L)][s] in (".", "X") else "open"
    lines = ["%-10s" % "slip" + "".join("%-10s" % k for k in APPLIES)]
    for s in SLIPS:
        lines.append("%-10s" % s + "".join("%-10s" % m[k][s] for k in APPLIES))
    return m, "\n".join(lines)


if __name__ == "__main__":
    print(kill_matrix()[1])
