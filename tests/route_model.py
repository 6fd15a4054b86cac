"""The launch routing restated in Python, from the comments of csrc/d2pc_route.hpp's call sites and DESIGN.md section 4 --
not from the header's code: which kernel serves a COMPACT call (`compact_plan`, and `route`, the view of it the
occupancy tests use) and how the fused COMPACT callback kernels cut a batch (`callback_plan`, `callback_route`).
tests/test_route_plan_cpu.py compares both with the header itself through tests/cpp/route_plan_main.cpp, on a CPU; the
GPU tests compare them with what the library did through d2pc_compact_stats.  No imports beyond the standard library."""
from collections import namedtuple

CU_DEFAULT = 256                   # an MI355X; the GPU tests read the device's own count
BLOCK = 256                        # threads per block: a tile is 256 * pxt ROI pixels
RESIDENT_BLOCKS_PER_CU = 4         # blocks of the resident forms (compact_algo 3) a CU holds at once
RESIDENT_TILES_PER_FRAME = 1024    # ... and the most tiles a frame may have for them
BIG_BATCH_FRAMES, BIG_BATCH_TILES = 4, 20480   # from here on the single pass serves by default
BLOCKS_PER_CU_DEFAULT = 128        # tuning "blocks_per_cu": the tile-walking grids
PIPE_BLOCKS_PER_CU_DEFAULT = 3     # tuning "callback_pipe_blocks_per_cu"; LDS and registers admit no more
CB_TILE_W, CB_TILE_H = 256, 32     # a tile of the fused callback kernels
CB_MAX_TILES_X = 128


# ---------------------------------------------------------------------------------------------------------------- COMPACT
def tiles_of(roi_n, pxt):
    return -(-roi_n // (BLOCK * pxt))


def walk_grid(total_tiles, cu, blocks_per_cu=BLOCKS_PER_CU_DEFAULT):
    """Many more blocks than fit, each walking a few tiles: min(T, max(CUs x blocks_per_cu, ceil(T / 4))), at least 1."""
    return max(1, min(total_tiles, max(cu * blocks_per_cu, -(-total_tiles // 4))))


def resident_fits(roi_n, n_frames, r, cu, unbounded=False):
    """Every tile of 256 * r pixels a block of its own, all of them resident at once, at most 1,024 to a frame.  The
    experiment `resident_unbounded` lifts both limits for the register-resident shapes (r >= 32) and the second for any."""
    tpf = tiles_of(roi_n, r)
    fits = tpf * n_frames <= cu * RESIDENT_BLOCKS_PER_CU or (unbounded and r >= 32 and tpf * n_frames <= 0x7FFFFFFF)
    return bool(fits and (tpf <= RESIDENT_TILES_PER_FRAME or unbounded))


def resident_shape(roi_n, n_frames, pxt, resident_pxt, cu, unbounded=False):
    """-> pixels per thread of the resident blocks, 0 if no shape fits: the caller's tiles, else 32, else 64; a forced
    `resident_pxt` serves where it fits and nothing else does in its place."""
    if resident_pxt:
        return resident_pxt if resident_fits(roi_n, n_frames, resident_pxt, cu, unbounded) else 0
    return next((r for r in (pxt, 32, 64) if resident_fits(roi_n, n_frames, r, cu)), 0)


def onepass_shape(roi_n, n_frames, pxt, onepass_form, onepass_blocks_per_cu, cu):
    """-> (form, pixels per thread, grid) of the single pass: forms 3 / 5 / 7 run on 4,096-pixel tiles with 2 blocks per
    CU, the other dense forms on 2,048-pixel tiles, form 1 on the caller's; 3 blocks per CU for frames of >= 2,048 tiles
    (4K), 4 for shorter ones; never more blocks than tiles."""
    form = onepass_form or 2
    big_tiles = form in (3, 5, 7)
    fp = 16 if big_tiles else 8 if form >= 2 else pxt
    per_cu = onepass_blocks_per_cu or (2 if big_tiles else 3 if tiles_of(roi_n, fp) >= 2048 else 4)
    return form, fp, min(tiles_of(roi_n, fp) * n_frames, cu * per_cu)


Served = namedtuple("Served", "algo pxt tiles form grid stagger self_clean")
CompactPlan = namedtuple("CompactPlan", "split algo pxt tiles form grid stagger self_clean")


def serve(algo, roi_n, n_frames, pxt=8, resident_pxt=0, onepass_form=0, cu=CU_DEFAULT, captured=False, force_algo=0,
          is_f32=True, blocks_per_cu=BLOCKS_PER_CU_DEFAULT, onepass_blocks_per_cu=0, big_batch_algo=2, unbounded=False,
          stagger_pct=-1):
    """ONE launch of the whole batch -> Served: the algorithm, its pixels per thread, its tiles, the single-pass form, the
    grid, whether the resident blocks start on a ramp, whether the launch cleans the idle half of its state."""
    total = tiles_of(roi_n, pxt) * n_frames
    big = n_frames >= BIG_BATCH_FRAMES and total >= BIG_BATCH_TILES
    rp = resident_shape(roi_n, n_frames, pxt, resident_pxt, cu, unbounded)
    if captured:                      # a captured launch's epoch would freeze in the graph
        rp = 0
    a = force_algo or algo or (big_batch_algo if big else 3 if rp else 1)
    if a == 3 and not rp:             # asked for, not possible here
        a = big_batch_algo if big else 1
    if a == 2:
        form, fp, grid = onepass_shape(roi_n, n_frames, pxt, onepass_form, onepass_blocks_per_cu, cu)
        if grid >= n_frames:
            return Served(2, fp, tiles_of(roi_n, fp) * n_frames, form, grid, False, form >= 2 and form != 4)
        a = 1                         # more frames than blocks: the two-pass form in the caller's tiles
    if a == 3:
        tiles = tiles_of(roi_n, rp) * n_frames
        # the ramped start: the register-resident blocks of ONE fp32 frame that fills >= 7/8 of the device; a tuned
        # percentage applies to every such launch (and 0 % switches it off)
        lean = rp != pxt
        ramp = lean and (stagger_pct > 0 if stagger_pct >= 0 else n_frames == 1 and is_f32 and tiles * 8 >= cu * RESIDENT_BLOCKS_PER_CU * 7)
        return Served(3, rp, tiles, 0, tiles, bool(ramp), False)
    if a == 4:                        # the chunked two-pass counts in its own 512-pixel tiles
        return Served(4, 2, tiles_of(roi_n, 2) * n_frames, 0, walk_grid(total, cu, blocks_per_cu), False, False)
    return Served(a, pxt, total, 0, walk_grid(total, cu, blocks_per_cu), False, False)


def route(algo, roi_n, n_frames, pxt=8, resident_pxt=0, onepass_form=0, cu=CU_DEFAULT):
    """-> (serving algorithm, its pixels per thread, its tiles per launch) for an eager launch of the whole batch (of >= 3
    frames, or a forced algorithm, or one that `compact_plan` does not split)."""
    s = serve(algo, roi_n, n_frames, pxt, resident_pxt, onepass_form, cu)
    return s.algo, s.pxt, s.tiles


def splits(algo, roi_n, n_frames, pxt=8, resident_pxt=0, cu=CU_DEFAULT, captured=False, force_algo=0, resident_pair=0):
    """TWO frames that fit the resident blocks only in blocks of 64 pixels per thread (two 4K frames) go as two launches
    of one frame each: an eager, unforced call under compact_algo 0 / 3 without a forced shape, whose single frame is
    resident in the caller's tiles or at 32 pixels per thread, and whose pair has too many blocks in both."""
    if n_frames != 2 or captured or force_algo or algo not in (0, 3) or resident_pxt or resident_pair:
        return False
    cap = cu * RESIDENT_BLOCKS_PER_CU
    single = resident_fits(roi_n, 1, pxt, cu) or resident_fits(roi_n, 1, 32, cu)
    return single and 2 * tiles_of(roi_n, pxt) > cap and 2 * tiles_of(roi_n, 32) > cap


def compact_plan(algo, roi_n, n_frames, pxt=8, resident_pxt=0, onepass_form=0, cu=CU_DEFAULT, captured=False, force_algo=0,
                 resident_pair=0, **kw):
    """The whole of a COMPACT call -> CompactPlan: split (then `launches(plan)` one-frame launches, each routed as
    compact_plan(..., n_frames=1)), or the one launch of `serve`."""
    if splits(algo, roi_n, n_frames, pxt, resident_pxt, cu, captured, force_algo, resident_pair):
        return CompactPlan(True, 0, 0, 0, 0, 0, False, False)
    return CompactPlan(False, *serve(algo, roi_n, n_frames, pxt, resident_pxt, onepass_form, cu, captured, force_algo, **kw))


# --------------------------------------------------------------------------------------------------------------- callback
CallbackSub = namedtuple("CallbackSub", "ns per_frame grid pipelined")
CallbackPlan = namedtuple("CallbackPlan", "resident nfc subs")
Route = namedtuple("Route", "n resident nfc per_frame tiles_x tiles_y tpf sub_batches pipelined")


def callback_tiles(roi_w, roi_h):
    return -(-roi_w // CB_TILE_W), -(-roi_h // CB_TILE_H)


def callback_plan(cu, per_cu, tiles_x, tiles_y, n, fused_form=2):
    """d2pc_process_mono_device's residency rule for the fused COMPACT forms.  A frame's blocks are dealt round-robin
    over the launch's frames and hand counts over inside a band, so a frame needs tiles_x blocks of its own resident:
    the batch goes in sub-batches of nfc frames with resident / nfc > tiles_x.  Form 2 gives every frame
    min(resident / ns, tiles per frame) persistent blocks where that is more than a band's tiles (or all the frame's
    tiles); otherwise, and under form 1, every tile has a block."""
    tpf = tiles_x * tiles_y
    resident = cu * min(per_cu, PIPE_BLOCKS_PER_CU_DEFAULT)
    nfc = max(resident // (tiles_x + 1), 1)
    subs = []
    for s0 in range(0, n, nfc):
        ns = min(n - s0, nfc)
        per_frame = min(resident // ns, tpf)
        pipelined = fused_form == 2 and (per_frame > tiles_x or per_frame == tpf)
        if not pipelined:
            per_frame = tpf
        subs.append(CallbackSub(ns, per_frame, per_frame * ns, pipelined))
    return CallbackPlan(resident, nfc, subs)


def callback_route(roi_w, roi_h, per_cu, aim, cu=CU_DEFAULT):
    """-> Route of the pipelined form for a ROI and a residency tuning.  n is chosen from the CU count so that a
    steady-state case gets about the per_frame it aims at (aim 0: n = 3)."""
    tiles_x, tiles_y = callback_tiles(roi_w, roi_h)
    tpf = tiles_x * tiles_y
    n = cu // aim if aim else 3
    resident = cu * min(per_cu, 3)
    nfc = max(resident // (tiles_x + 1), 1)
    ns = min(n, nfc)                                        # the first sub-batch
    per_frame = min(resident // ns, tpf)
    return Route(n, resident, nfc, per_frame, tiles_x, tiles_y, tpf, -(-n // nfc), per_frame > tiles_x or per_frame == tpf)


def callback_overlap(cb_chunks, width, height, n_frames, median, bridge16, captured):
    """-> (overlap, frames per chunk).  Few, large chunks: the batch is cut (at most one chunk per frame) only for an
    eager call with a filter or a rescale in front, and only when every chunk carries at least 16 Mi pixels."""
    chunks = min(cb_chunks, n_frames)
    overlap = chunks > 1 and not captured and (median or bridge16) and width * height * n_frames // chunks >= 16 << 20
    return bool(overlap), -(-n_frames // chunks) if overlap else n_frames


def callback_one_kernel(overlap, median, cb_fused, cb_fused_compact, compact, bs_median, roi_w):
    """Filter and points tile by tile in one kernel: a median call in order on one stream whose filter launch would be
    the bit-sliced one; COMPACT needs a fused form switched on and a band of at most 128 tiles."""
    ok = median and cb_fused == 1 and not overlap and bs_median
    if compact:
        ok = ok and cb_fused_compact >= 1 and -(-roi_w // CB_TILE_W) <= CB_MAX_TILES_X
    return bool(ok)
