"""The fusion kernels on built inputs (tests/fusion_patterns.py; tests/README.md, "Fusion patterns"): every rule's
k_fuse_median3<RULE, NARROW> at its thresholds, in every byte lane and across its strip and chunk seams, and the
single-launch k_node_fuse<16|64> on GRAD_FILTER's table and on seam patterns laid out for its tiles.  The expected answer
is oracle.fuse (and colorize_ref.colorize for the node's colour topics), byte for byte.

Every k_fuse_median3 case launches from one arena of sentinel bytes that holds the input planes (each with its own pitch,
base alignment and frame stride, guard rows and columns around it) into another that holds the outputs; afterwards the
input arena is unchanged and the output arena is all sentinel again once the planes themselves are blanked.

Cut from the cross product (about 20 s for the file was the budget):
  * the geometry cases run per rule in one test, not one test per (rule, shape): 123 shapes x 17 would be pytest overhead;
  * median_edges runs at every size, fuse_rows and crop case, but not on the three-frame layout cases and the
    1,241 x 5 x 2 case, whose frame counts are the point: lively runs there;
  * the combined plane alternates with the case index instead of doubling the cases (rule_table runs both);
  * the node runs GRAD_FILTER only (it has no other single-launch kernel), its table with a zero crop, the seam patterns
    at n = 192 with three crops, and one 16-frame batch of n = 736 for the 64-row tile.
"""
import numpy as np
import pytest
import torch

import disparity_to_point_cloud_amd as d2pc
from disparity_to_point_cloud_amd import capi
import oracle
import fusion_patterns as fp
from test_fusion_session_gpu import _fuse_planes

pytestmark = pytest.mark.gpu

WIDTHS = (1, 2, 3, 4, 5, 7, 8, 247, 248, 249, 251, 252, 496, 497)
HEIGHTS = (1, 2, 3, 4, 5, 7)
FUSE_ROWS = (0, 2, 4, 6, 16)
REFERENCE_CROP = (0, 40, 30, 10)


def _geometry():
    """name, h, w, frames, crop (l, r, t, b), fuse_rows, layout (pads, shifts, score1 is grad1) or None, median_edges too."""
    cases = []
    add = lambda name, h, w, frames=1, crop=(0, 0, 0, 0), rows=0, layout=None, edges=True: cases.append(  # noqa: E731
        dict(name=name, h=h, w=w, frames=frames, crop=crop, rows=rows, layout=layout, edges=edges,
             combined=len(cases) % 2 == 0))
    for w in WIDTHS:
        for h in HEIGHTS:
            add("size", h, w)
    for r in FUSE_ROWS:  # two strips; a chunk short of, on and past r rows, two chunks and a row, 4k + 2 rows
        for h in sorted({h for h in (r - 1, r, r + 1, 2 * r + 1, 4 * r + 2) if h >= 1}):
            add("fuse_rows", h, 249, rows=r)
    for k, crop in enumerate([(1, 2, 1, 1), (2, 1, 0, 2), (3, 0, 2, 0), (4, 3, 1, 0), (5, 7, 0, 0), (246, 1, 0, 0),
                              (247, 0, 3, 2), (248, 4, 0, 8), (250, 2, 1, 1), (0, 0, 4, 4), (249, 3, 5, 3)]):
        add("crop", 9, 253, crop=crop, rows=(0, 4)[k % 2])  # (250, 2, ..): one pixel wide; (0, 0, 4, 4): one high; last: 1 x 1
    add("crop", 43, 249, crop=REFERENCE_CROP)
    add("seams", 31, 500)  # 496 is no border column; tall enough for the ten count blocks of a seam column in one column of blocks
    layout = ((0, 1, 2, 3, 5, 8), (0, 1, 2, 3, 1, 2), True)
    add("layout", 7, 251, frames=3, layout=layout, edges=False)
    add("layout", 5, 3, frames=3, layout=layout, edges=False)
    add("layout", 6, 497, frames=3, crop=(3, 2, 1, 1), layout=((9, 4, 0, 1, 2, 3), (3, 2, 1, 0, 3, 1), True), edges=False)
    # six strips x two chunks x two frames = 24 waves: a block's four waves lie in different chunks and frames
    add("six_strips", 5, 1241, frames=2, edges=False)
    for c in cases:
        c["combined"] = c["combined"] or c["layout"] is not None
    return cases


GEOMETRY = _geometry()
TABLE_CASES = [(rule, combined) for rule in fp.RULES for combined in (True, False)]
# the node: cols = rows = n; (n, crop, batch) -- tile columns 63|64 and 127|128, tile rows 15|16 (16-row tiles) and 63|64
NODE_SEAMS = dict(seams_x=(63, 64, 127, 128), seams_y=(15, 16, 63, 64))
NODE_CASES = [(192, (0, 40, 30, 10)), (192, (64, 2, 16, 3)), (192, (63, 3, 15, 17))]
NODE_TALL = (736, 16)


def case_seed(rule, k):
    return 1000 * rule + k


def lively_planes(rule, case, k):
    """The six (F, h, w) planes of a lively case: the generator per frame, seeded gradients (score1's own plane where the
    layout aliases them)."""
    rng = np.random.default_rng(case_seed(rule, k))
    frames = [fp.lively(rule, rng, case["h"], case["w"]) for _ in range(case["frames"])]
    planes = [np.stack([f[p] for f in frames]) for p in range(4)]
    g = [rng.integers(0, 256, size=planes[0].shape).astype(np.uint8) for _ in range(2)]
    return planes + g


def edge_planes(rule, case):
    planes = fp.median_edges(rule, case["h"], case["w"])
    return planes + [planes[3], planes[0]]


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q()) as c:
        yield c


def _view(arena, spec, frames, rows, width):
    base, pitch, stride = spec
    return np.lib.stride_tricks.as_strided(arena[base:], shape=(frames, rows, width), strides=(stride, pitch, 1))


def run_case(ctx, rule, planes, crop=(0, 0, 0, 0), combined=True, layout=None, what=None):
    """Launch d2pc_fuse_device on (F, h, w) planes laid into a sentinel arena; outputs into another; compare."""
    pads, shifts, alias = layout or ((3, 0, 5, 1, 2, 4), (0, 0, 0, 0, 0, 0), False)
    frames, h, w = planes[0].shape
    n_in = 6 if combined else 4
    specs, cursor = [], 64
    for p in range(n_in):
        if alias and p == 4:
            specs.append(specs[2])
            continue
        pitch = w + pads[p]
        base = (cursor + pitch + 3) // 4 * 4 + shifts[p]          # base alignment = shifts[p] mod 4
        stride = pitch * (h + 2) + p                               # no multiple of the pitch
        specs.append((base, pitch, stride))
        cursor = base + frames * stride + pitch + 64
    host = np.full(cursor, fp.SENTINEL, dtype=np.uint8)
    for p in range(n_in):
        _view(host, specs[p], frames, h, w)[...] = planes[2 if alias and p == 4 else p]
    dev_in = torch.from_numpy(host).cuda()
    l, r, t, b = crop
    oh, ow = h - t - b, w - l - r
    f_spec = (64 + 2 * (ow + 5) + 1, ow + 5, (ow + 5) * (oh + 3) + 1)
    end = f_spec[0] + frames * f_spec[2] + 2 * (ow + 5) + 64
    c_spec = (end + 2 * (w + 7) + 3, w + 7, (w + 7) * (h + 2) + 3)
    if combined:
        end = c_spec[0] + frames * c_spec[2] + 3 * (w + 7) + 64
    dev_out = torch.full((end,), fp.SENTINEL, dtype=torch.uint8, device="cuda")
    desc = capi.fuse_desc_init()
    desc.rule, desc.width, desc.height, desc.n_frames = rule, w, h, frames
    desc.crop_left, desc.crop_right, desc.crop_top, desc.crop_bottom = l, r, t, b
    for p in range(n_in):
        desc.planes[p] = dev_in.data_ptr() + specs[p][0]
        desc.pitch[p], desc.frame_stride[p] = specs[p][1], specs[p][2]
    desc.fused, desc.fused_pitch, desc.fused_frame_stride = dev_out.data_ptr() + f_spec[0], f_spec[1], f_spec[2]
    if combined:
        desc.combined = dev_out.data_ptr() + c_spec[0]
        desc.combined_pitch, desc.combined_frame_stride = c_spec[1], c_spec[2]
    ctx.fuse_device(desc, torch.cuda.current_stream().cuda_stream)
    out = dev_out.cpu().numpy()
    assert np.array_equal(dev_in.cpu().numpy(), host), (what, "an input changed")
    got_f = _view(out, f_spec, frames, oh, ow).copy()
    got_c = _view(out, c_spec, frames, h, w).copy() if combined else None
    for f in range(frames):
        one = [np.ascontiguousarray(planes[p][f]) for p in range(6 if combined else 4)]
        if alias and combined:
            one[4] = one[2]
        want_f, want_c = oracle.fuse(one + [one[0]] * (6 - len(one)), rule=rule, crop=crop, want_combined=combined)
        assert np.array_equal(got_f[f], want_f), (what, f, "fused", int((got_f[f] != want_f).sum()),
                                                  np.argwhere(got_f[f] != want_f)[:4].tolist())
        if combined:
            assert np.array_equal(got_c[f], want_c), (what, f, "combined", np.argwhere(got_c[f] != want_c)[:4].tolist())
    _view(out, f_spec, frames, oh, ow)[...] = fp.SENTINEL
    if combined:
        _view(out, c_spec, frames, h, w)[...] = fp.SENTINEL
    assert (out == fp.SENTINEL).all(), (what, "bytes outside the output planes changed", np.flatnonzero(out != fp.SENTINEL)[:4])


# ---- k_fuse_median3 ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rule,combined", TABLE_CASES)
def test_rule_table(ctx, rule, combined):
    """Every rule at S x S scores around its own thresholds x the edge distances, and all 65,536 distance pairs per
    outcome class -- the WHOLE image compared, so cell borders (two to four cells in a window) count too."""
    ctx.set_tuning("fuse_rows", 0)
    for name, planes in fp.rule_table(rule):
        six = [p[None] for p in planes] + [planes[2][None], planes[1][None]]
        run_case(ctx, rule, six, combined=combined, what=(fp.RULE_NAMES[rule], name))


def _geometry_cases(ctx, rule, which):
    for k, case in enumerate(GEOMETRY):
        if which == "edges" and not case["edges"]:
            continue
        planes = lively_planes(rule, case, k) if which == "lively" else edge_planes(rule, case)
        ctx.set_tuning("fuse_rows", case["rows"])
        try:
            run_case(ctx, rule, planes, crop=case["crop"], combined=case["combined"], layout=case["layout"],
                     what=(fp.RULE_NAMES[rule], which, k, {n: case[n] for n in ("name", "h", "w", "crop", "rows")}))
        finally:
            ctx.set_tuning("fuse_rows", 0)


@pytest.mark.parametrize("rule", fp.RULES)
def test_geometry_lively(ctx, rule):
    """Every rule's kernel on images with structure (every outcome class at 10 % of the pixels or more): widths 1..3
    (NARROW), around one and two strips, heights 1..7, every fuse_rows against chunks short of, on and past it, crops
    from every column mod 4, one-pixel maps, pitched and misaligned planes in batches, six strips."""
    _geometry_cases(ctx, rule, "lively")


@pytest.mark.parametrize("rule", fp.PASS_THROUGH)
def test_geometry_median_edges(ctx, rule):
    """Two-level planes handed through the rule to the median: windows of 0..9 high pixels on the seam columns, single
    pixels beside every border and seam in every byte lane, stripes and a checkerboard."""
    _geometry_cases(ctx, rule, "edges")


# ---- k_node_fuse ------------------------------------------------------------------------------------------------------
def test_node_rule_table(ctx):
    """GRAD_FILTER's table through the single launch (16-row tiles) and the three-launch composition, all four topics."""
    for name, planes in fp.rule_table(fp.GRAD_FILTER):
        if name == "edges_narrow":
            continue
        n = planes[0].shape[0]
        _fuse_planes(ctx, n, n, 0, 0, *[p[None] for p in planes], crop=(0, 0, 0, 0))


@pytest.mark.parametrize("n,crop", NODE_CASES)
def test_node_seams(ctx, n, crop):
    """The seam patterns laid out for the node's units: tile columns 63|64 and 127|128, tile rows 15|16 and 63|64, the
    crop starting on a tile's first and last column."""
    planes = fp.median_edges(fp.GRAD_FILTER, n, n, **NODE_SEAMS)
    _fuse_planes(ctx, n, n, 0, 0, *planes, batch=planes[0].shape[0], crop=crop)
    rng = np.random.default_rng(n + crop[0])
    _fuse_planes(ctx, n, n, 0, 0, *[p[None] for p in fp.lively(fp.GRAD_FILTER, rng, n, n)], crop=crop)


def test_node_tall_tiles(ctx):
    """2,048 tall tiles and more select the 64-row tile: 16 frames of n = 736, built from the seam patterns."""
    n, batch = NODE_TALL
    assert (-(-n // 64)) ** 2 * batch >= 2048
    planes = fp.median_edges(fp.GRAD_FILTER, n, n, **NODE_SEAMS)
    pick = np.linspace(0, planes[0].shape[0] - 1, batch).astype(int)  # stripes, count blocks, bright and dark singles
    planes = [np.ascontiguousarray(p[pick]) for p in planes]
    lively = fp.lively(fp.GRAD_FILTER, np.random.default_rng(736), n, n)
    for p in range(4):
        planes[p][batch - 1] = lively[p]
    _fuse_planes(ctx, n, n, 0, 0, *planes, batch=batch)
