"""tests/address_patterns.py reaches what it was built to reach -- at the geometries tests/test_address_range_gpu.py
uses.  No GPU, nothing large: a layout is eight integers."""
import os
import re

import numpy as np
import pytest

import address_patterns as ap
from address_patterns import G, H

GEOMS = ap.gpu_geometries()
IDS = ["%s-%s" % (L.name, re.sub(r"[^0-9a-z]+", "_", s.lower())) for s, L in GEOMS]
ARENA_CAP = int(6.5 * (1 << 30))
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def of(*families):
    return [pytest.param(s, L, id=i) for (s, L), i in zip(GEOMS, IDS) if ap.family(L) in families]


def test_every_kind_is_used_on_the_gpu():
    assert {L.name for _, L in GEOMS} == set(ap.KINDS) - {"dense"}
    assert set(ap.APPLIES) == {ap.family(k) for k in ap.KINDS}


@pytest.mark.parametrize("subject,L", of("far", "straddle", "tall", "high"))
def test_layout_is_sound(subject, L):
    """Rows lie inside the arena, in order and apart; the arena keeps to its cap (the index plane past 4 GiB is the
    one exception the GPU file allows itself)."""
    t = ap.touched(L)
    assert ap.inside_arena(L)
    flat = t.reshape(-1, 2)
    assert np.all(flat[1:, 0] >= flat[:-1, 1]), "rows overlap or are out of order"
    assert L.pitch >= L.row_bytes and (L.n_frames == 1 or L.frame_stride >= L.rows * L.pitch)
    if "index plane" not in subject:
        assert L.arena_bytes <= ARENA_CAP
    else:
        assert L.arena_bytes * 4 > 16 * (1 << 30)   # (its points, 16 bytes a record, are the 16 GiB arena)


@pytest.mark.parametrize("subject,L", of("far"))
def test_far_puts_frame_1_wholly_above_4_gib(subject, L):
    off = ap.row_offsets(L)
    assert L.n_frames == 2 and off[1].min() >= G
    cut = L.frame_stride % G
    assert 0 < cut <= 8192, "the stride cut to 32 bits lands near frame 0"
    if L.name == "far16":
        assert L.base % 16 == 0 and L.frame_stride % 16 == 0 and (L.pitch % 16 == 0 or L.pitch == L.row_bytes)   # (or packed records)
    else:
        assert L.base % 16 and L.pitch % 16 and L.frame_stride % 16


@pytest.mark.parametrize("subject,L", of("straddle"))
def test_straddle_puts_offset_4_gib_inside_frame_1(subject, L):
    lo = L.frame_stride
    assert L.n_frames == 2 and lo < G < lo + ap.frame_extent(L)
    assert L.frame_stride < G   # (so frame32 does not apply; sum32 does)
    assert abs((G - lo) - ap.frame_extent(L) // 2) <= 128, "2^32 falls in the middle of the frame"


@pytest.mark.parametrize("subject,L", of("tall"))
def test_tall_has_rows_either_side_of_4_gib(subject, L):
    off = ap.row_offsets(L)[0]
    assert L.n_frames == 1 and L.rows * L.pitch > G + L.pitch
    assert (off >= G).sum() >= 2, "at least two rows start above 4 GiB"
    below = off[off < G].max()
    assert G - below <= L.pitch, "one row starts just below it"
    assert abs(L.pitch - (1 << 26)) < 64 and L.pitch % 2 == (0 if "mono16" in subject else 1)
    assert L.pitch <= 0xFFFFFFFF
    assert ((off % G >= H) & (off < G)).any(), "row offsets that an int turns negative"


@pytest.mark.parametrize("subject,L", of("high"))
def test_high_sits_on_the_host_limit(subject, L):
    off = ap.row_offsets(L)[0]
    assert L.n_frames == 1 and L.base == H and off.max() + L.row_bytes <= 0xFFFFFFFF
    assert (off >= H).sum() >= L.rows // 3, "the last third of the rows starts above 2^31"
    assert np.all(off[-(L.rows // 3):] >= H)
    if "process_device" in subject:
        p = ap.HIGH_PROCESS
        assert (L.rows, L.pitch, L.row_bytes) == (p["height"], p["row_stride"], p["width"] * p["elem"])
        assert (p["height"] + 4097) * p["row_stride"] < G
        assert ap.geom_fits(p["width"], L.rows, L.pitch, 0, 1, p["elem"])
        # the largest row stride make_geom takes for these rows, in steps of the element ...
        assert not ap.geom_fits(p["width"], L.rows, L.pitch + p["elem"], 0, 1, p["elem"])
        assert L.pitch == (0xFFFFFFFF // (L.rows + 4097)) // p["elem"] * p["elem"]
        # ... and a 16-column ROI at border 40, 981,760 points
        assert p["width"] - 2 * p["border"] == 16 and 16 * (L.rows - 2 * p["border"]) == 981760
    else:
        assert ap.plane_fits(L.pitch, 0, L.rows, L.row_bytes, 1, "plane")
        assert not ap.plane_fits(L.pitch + 1, 0, L.rows, L.row_bytes, 1, "plane"), "one byte of pitch more is refused"
        assert not ap.plane_fits(L.pitch, 0, L.rows + 1, L.row_bytes, 1, "plane"), "one row more is refused"
        assert L.pitch == ap.plane_max_pitch(L.rows)


def test_pitch_bound_is_the_pitch_alone():
    """Bound32::Pitch: any pitch below 2^32 whatever the rows (so `tall` is accepted), 2^32 refused."""
    assert ap.plane_fits(0xFFFFFFFF, 0, 70, 203, 1, "pitch") and not ap.plane_fits(G, 0, 70, 203, 1, "pitch")
    L = ap.tall(70, 203)
    assert ap.plane_fits(L.pitch, 0, L.rows, L.row_bytes, 1, "pitch") and not ap.plane_fits(L.pitch, 0, L.rows, L.row_bytes, 1, "plane")


# ---------------------------------------------------------------------------------------------------- the kill matrix
@pytest.mark.parametrize("subject,L", of("far", "straddle", "tall", "high"))
def test_every_applicable_slip_is_killed_inside_the_arena(subject, L):
    """For each slip that applies: the slipped rows differ from the true ones, every slipped byte lies inside the
    arena (the comparison fails; nothing faults), and no slipped frame lands exactly on another frame."""
    assert ap.APPLIES[ap.family(L)]
    for slip in ap.APPLIES[ap.family(L)]:
        assert ap.killed(L, slip), slip
        assert ap.inside_arena(L, slip), slip
        assert not ap.coincides_with_another_frame(L, slip), slip
        moved = np.any(ap.touched(L, slip) != ap.touched(L), axis=(1, 2))
        if ap.family(L) in ("far", "straddle"):
            assert moved[1] and not moved[0]   # frame 0 is where it belongs, frame 1 is not


@pytest.mark.parametrize("subject,L", of("far", "straddle", "tall", "high"))
def test_slips_that_do_not_apply_change_nothing(subject, L):
    """The matrix's dots are real: a slip left out of APPLIES moves no row of that layout, so the layout cannot show it
    (`high`: offsets stay below 2^32 by the host's rule; `far` and `straddle`: no row offset of their small frames
    reaches 2^31; `straddle`: its stride is below 2^32; `tall`: one frame)."""
    for slip in set(ap.SLIPS) - set(ap.APPLIES[ap.family(L)]):
        assert not ap.killed(L, slip), slip


def test_dense_shows_no_slip():
    L = ap.dense(131, 203, 2)
    assert all(not ap.killed(L, s) for s in ap.SLIPS)


def test_kill_matrix_is_the_one_in_the_readme():
    m, text = ap.kill_matrix()
    for fam, slips in ap.APPLIES.items():
        for s in ap.SLIPS:
            assert m[fam][s] == ("X" if s in slips else "."), (fam, s)
    with open(os.path.join(ROOT, "tests", "README.md")) as f:
        assert text in f.read()
