"""Ordered compaction on built occupancy patterns (tests/occupancy_patterns.py) through every compaction path, and the
tile-count ladder across the seams the code branches on.  What each pattern reaches and the kill matrix of the numpy
model are asserted without a GPU in tests/test_occupancy_patterns.py, at exactly the cases of `CASES`, `PATHS` and
`LADDER` below; `case_of` refuses anything else.

Every pattern case runs every path of `paths_for(case)`:

  product build     compact_algo 1 (two-pass), 2 (single pass, form 2), 3 (resident: the router's shape, and the lean
                    blocks of 32 / 64 pixels per thread forced), 0 (default routing) on the case's own batch and on a batch
                    repeated to either side of the big-batch rule (4 frames and 20,480 tiles); f32 with and without 16-byte
                    row loads, u8 and u16 input; with and without indices; the three hole kinds
  experiment build  compact_algo 4 (chunked two-pass); a sample of the single-pass forms 1 and 3-7; pxt_compact 4 / 16

The matrix is thinned, the patterns are not.  CUT: (algorithm x dtype x index x hole kind x row loads) is not a full
product -- each algorithm meets f32 with indices, one or two of {no indices, no 16-byte loads, u8, u16} and two or
three of the hole kinds, and every case meets all three kinds, both index settings, both row-load settings and all three
dtypes across its paths (asserted on the CPU); the experiment forms 1, 4 and 6 run f32 only, one hole kind and one index
setting each (rotating with the case); tile sizes 1,024 / 4,096 (pxt_compact 4 / 16, forms 1 / 3 / 5 / 7) run the
thinned case list of make_cases(tile, thin=True), one to three cases per generator, three to five paths each (every form
still meets every generator); the big-batch pair runs f32 with indices only.

Checking: helpers.check_compact_is_filtered_parity (counts, indices and point bits equal the same context's PARITY
output filtered on the host; no give-up; the launch counters name the algorithm that served), then idx == pix[valid]
from the mask itself, then a SECOND launch into buffers filled with sentinel bits: equal to the first in the first
`count` entries, and every word from `count` to the stride still the sentinel.  One path per case also goes against
oracle.reproject_compact in OpenCV 2.4's form.  Big batches and the ladder are compared on the device with torch
(device_check) and bring back only counts and verdicts."""
from collections import namedtuple

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import occupancy_patterns as op
import oracle
from helpers import check_compact_is_filtered_parity
from route_model import BIG_BATCH_TILES, route     # the router, restated: compared with the C++ on a CPU by test_route_plan_cpu.py

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PT_SENTINEL, IX_SENTINEL = 0x7FC5A5A5, 0x5A5AA5A5   # a NaN with a payload no kernel produces; an index beyond any frame

CASES = {2048: op.make_cases(2048), 1024: op.make_cases(1024, thin=True), 4096: op.make_cases(4096, thin=True)}

Path = namedtuple("Path", "name algo exp dtype vec idx kind tune tile batch oracle")


def _p(name, algo, dtype="f32", vec=True, idx=True, kind="zero", exp=False, tune=(), tile=2048, batch="own", oracle_form=False):
    return Path(name, algo, exp or algo == 4 or tile != 2048, dtype, vec, idx, kind, tuple(tune), tile, batch, oracle_form)


PRODUCT_PATHS = [
    _p("a1", 1, kind="zero", oracle_form=True),
    _p("a1_scalar_noidx", 1, vec=False, idx=False, kind="nan"),
    _p("a1_u8_noidx_floor", 1, dtype="u8", idx=False, kind="floor"),
    _p("a2", 2, kind="nan"),
    _p("a2_scalar_noidx_floor", 2, vec=False, idx=False, kind="floor"),
    _p("a2_u8", 2, dtype="u8", kind="zero"),
    _p("a2_u16_noidx", 2, dtype="u16", idx=False, kind="zero"),
    _p("a3", 3, kind="floor"),
    _p("a3_r32", 3, kind="zero", tune=(("resident_pxt", 32),)),
    _p("a3_r64_noidx", 3, idx=False, kind="nan", tune=(("resident_pxt", 64),)),
    _p("a3_r32_u16_floor", 3, dtype="u16", kind="floor", tune=(("resident_pxt", 32),)),
    _p("a0", 0, kind="zero"),
    _p("a0_scalar_nan", 0, vec=False, kind="nan"),
    _p("a0_big", 0, kind="nan", batch="big"),
    _p("a0_below_big", 0, kind="floor", batch="below_big"),
]
EXP_PATHS = [
    _p("a4", 4, kind="zero"),
    _p("a4_scalar_nan", 4, vec=False, kind="nan"),
    _p("a4_u8_noidx_floor", 4, dtype="u8", idx=False, kind="floor"),
]
FORMS_2048 = (1, 4, 6)       # single-pass forms on 2,048-pixel tiles (form 1: the tile shape of pxt_compact)
FORMS_4096 = (3, 5, 7)       # ... on 4,096-pixel tiles


def paths_for(case):
    i = [c.name for c in CASES[case.tile]].index(case.name)
    kinds = op.HOLE_KINDS
    if case.tile == 2048:
        return PRODUCT_PATHS + EXP_PATHS + [
            _p(f"a2_form{f}", 2, exp=True, kind=kinds[(i + j) % 3], idx=bool((i + j) % 2), tune=(("onepass_form", f),)) for j, f in enumerate(FORMS_2048)]
    if case.tile == 4096:
        return [_p("a1_pxt16", 1, kind="nan", tile=4096, tune=(("pxt_compact", 16),)),
                _p("a3_pxt16_noidx", 3, idx=False, kind="floor", tile=4096, tune=(("pxt_compact", 16),)),
                _p("a2_form3", 2, kind="zero", tile=4096, tune=(("onepass_form", 3),)),
                _p("a2_form5_noidx", 2, idx=False, kind="nan", tile=4096, tune=(("onepass_form", 5),)),
                _p("a2_form7_u8", 2, dtype="u8", kind="floor", tile=4096, tune=(("onepass_form", 7),))]
    return [_p("a1_pxt4", 1, kind="floor", tile=1024, tune=(("pxt_compact", 4),)),
            _p("a3_pxt4_u16", 3, dtype="u16", kind="zero", tile=1024, tune=(("pxt_compact", 4),)),
            _p("a2_form1_pxt4_noidx", 2, idx=False, kind="nan", tile=1024, tune=(("pxt_compact", 4), ("onepass_form", 1)))]


PATTERN_TESTS = [(c, p) for tile in (2048, 1024, 4096) for c in CASES[tile] for p in paths_for(c)]


def case_of(tile, name):
    """Only the cases whose reach tests/test_occupancy_patterns.py asserts are run."""
    for c in CASES[tile]:
        if c.name == name:
            return c
    raise AssertionError(f"{name}@{tile} is not a case of CASES: its reach is asserted nowhere")


# --------------------------------------------------------------------------------------------------------------- contexts
_ctx = {}
TUNING_DEFAULTS = (("onepass_form", 0), ("resident_pxt", 0), ("no_vec_rows", 0), ("pxt_compact", 8), ("onepass_blocks_per_cu", 0))


def ctx_for(algo, exp, tune=(), vec=True):
    key = (algo, "exp" if exp else None)
    if key not in _ctx:
        _ctx[key] = d2pc.Context(q=d2pc.make_q(), mode=d2pc.MODE_COMPACT, compact_algo=algo, variant=key[1])
    c = _ctx[key]
    c.set_mode(d2pc.MODE_COMPACT)
    c.set_reproject_form(d2pc.FORM_DEFAULT)
    c.set_min_disparity(-np.inf)
    for k, v in TUNING_DEFAULTS:
        c.set_tuning(k, v)
    for k, v in tune:
        c.set_tuning(k, v)
    if not vec:
        c.set_tuning("no_vec_rows", 1)
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    torch.cuda.reset_peak_memory_stats()
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    _rung.clear()            # (the last rung's frame and mask: nothing of this module stays on the device)
    torch.cuda.empty_cache()
    print("\npeak device memory of test_compact_occupancy_gpu.py: %.3f GiB" % (torch.cuda.max_memory_allocated() / 2**30))


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def assert_counters(st0, st, served, tiles, launches, what):
    """Between two readings of d2pc_compact_stats: nothing gave up and nothing was rerun by the two-pass form, whatever
    the algorithm; the single pass (2) and the resident blocks (3) counted `launches` launches of `tiles` tiles each,
    the two-pass forms (1, 4) none."""
    assert st["timeouts"] == st0["timeouts"] and st["twopass_fallbacks"] == st0["twopass_fallbacks"], (what, st0, st)
    if served in (2, 3):
        assert st["launches"] == st0["launches"] + launches, (what, st0, st)
        assert st["tiles"] == st0["tiles"] + launches * tiles, (what, st0, st, tiles)
    else:
        assert st["launches"] == st0["launches"] and st["tiles"] == st0["tiles"], (what, st0, st)


# ------------------------------------------------------------------------------------------------------------ device check
def device_check(ctx, disp, valid, border, want_index, served, tiles, launches=2, dmin=-np.inf, what=""):
    """disp (n, h, w) and valid (n, roi_n) on the device.  PARITY once, COMPACT `launches` times into buffers of sentinel
    bits; on the device: counts == valid.sum(), isfinite(PARITY) & !(d <= min_disparity) == valid, points == PARITY[valid] bit for bit in frame
    and ROI order, indices == pix[valid], every word from count to the stride still the sentinel; the counters show
    that `served` took the launches (and, where it counts them, `tiles` tiles each) and nothing gave up."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    n, h, w = disp.shape
    b = DeviceBatch(ctx, n, h, w, dtype=disp.dtype, want_index=want_index)
    b.disp.copy_(disp)
    roi_n = b.roi_n
    assert valid.shape == (n, roi_n)
    ctx.set_mode(d2pc.MODE_PARITY)
    b.launch()
    torch.cuda.synchronize()
    ctx.check_async_error()
    full = b.points[:, :roi_n]
    finite = torch.isfinite(full[:, :, :3]).all(dim=2)
    if dmin > -np.inf:
        finite &= ~(disp[:, border:h - border, border:w - border].reshape(n, roi_n) <= dmin)
    assert torch.equal(finite, valid), what + ": PARITY is finite (and above the floor) exactly where the mask says"
    want_pts = full.view(torch.int32)[valid]        # frame-major, ROI order
    del full, finite
    want_n = valid.sum(dim=1).to(torch.int32)
    ctx.set_mode(d2pc.MODE_COMPACT)
    st0 = ctx.compact_stats()
    pos = torch.arange(b.stride, device=disp.device)[None, :]
    for launch in range(launches):
        b.points.view(torch.int32).fill_(PT_SENTINEL)
        if want_index:
            b.index.fill_(IX_SENTINEL)
        b.counts.fill_(-7)
        b.launch()
        torch.cuda.synchronize()
        ctx.check_async_error()
        counts = b.counts.cpu().numpy().view(np.uint32)
        assert not np.any(counts == 0xFFFFFFFF), f"{what} launch {launch}: a frame was given up"
        assert np.array_equal(counts, want_n.cpu().numpy().view(np.uint32)), f"{what} launch {launch}: counts {counts}"
        head = pos < b.counts[:, None]
        pts = b.points.view(torch.int32)
        assert torch.equal(pts[head], want_pts), f"{what} launch {launch}: points"
        assert bool((pts[~head] == PT_SENTINEL).all()), f"{what} launch {launch}: a point beyond the count was written"
        if want_index:
            rv, ru = torch.div(torch.arange(roi_n, device=disp.device), w - 2 * border, rounding_mode="floor"), None
            ru = torch.arange(roi_n, device=disp.device) - rv * (w - 2 * border)
            pix = ((rv + border) * w + ru + border).to(torch.int32)
            want_idx = pix[None, :].expand(n, roi_n)[valid]
            assert torch.equal(b.index[head], want_idx), f"{what} launch {launch}: indices"
            assert bool((b.index[~head] == IX_SENTINEL).all()), f"{what} launch {launch}: an index beyond the count was written"
            del want_idx, pix, rv, ru
        del head, pts
    assert_counters(st0, ctx.compact_stats(), served, tiles, launches, what)


# ----------------------------------------------------------------------------------------------------------- the patterns
def second_launch_keeps_the_sentinels(ctx, data, first, want_index, served, tiles, what):
    """The batch again, into buffers of sentinel bits: the first `count` entries as the first launch left them, every
    word from there to the stride untouched (the stride padding included); the counters as for the first launch --
    nothing gave up, no two-pass rerun, `served` took the launch (and, where it counts them, `tiles` tiles)."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    pts1, idx1, counts1 = first
    frames = data.frames
    n, (h, w) = len(frames), frames[0].shape
    tdt = {np.dtype(np.float32): torch.float32, np.dtype(np.uint8): torch.uint8, np.dtype(np.uint16): torch.uint16}[frames[0].dtype]
    b = DeviceBatch(ctx, n, h, w, dtype=tdt, want_index=want_index)
    stack = np.stack(frames)
    b.disp.copy_(torch.from_numpy(stack.view(np.int16)).view(tdt) if stack.dtype == np.uint16 else torch.from_numpy(stack))
    b.points.view(torch.int32).fill_(PT_SENTINEL)
    if want_index:
        b.index.fill_(IX_SENTINEL)
    b.counts.fill_(-7)
    st0 = ctx.compact_stats()
    b.launch(scale=data.scale)
    torch.cuda.synchronize()
    ctx.check_async_error()
    assert_counters(st0, ctx.compact_stats(), served, tiles, 1, what + ": second launch")
    counts = b.counts.cpu().numpy().view(np.uint32)
    assert not np.any(counts == 0xFFFFFFFF), what
    assert np.array_equal(counts, counts1), what
    pts = b.points.cpu().numpy().view(np.uint32)
    idx = b.index.cpu().numpy().view(np.uint32) if want_index else None
    for f in range(n):
        c = int(counts[f])
        assert np.array_equal(pts[f, :c], pts1[f, :c].view(np.uint32)), f"{what} frame {f}: second launch"
        assert np.all(pts[f, c:] == PT_SENTINEL), f"{what} frame {f}: a point beyond the count was written"
        if want_index:
            assert np.array_equal(idx[f, :c], idx1[f, :c]), f"{what} frame {f}: second launch, indices"
            assert np.all(idx[f, c:] == IX_SENTINEL), f"{what} frame {f}: an index beyond the count was written"


@pytest.mark.parametrize("case,path", PATTERN_TESTS, ids=[f"{c.name}@{c.tile}-{p.name}" for c, p in PATTERN_TESTS])
def test_occupancy_patterns_through_every_compaction_path(case, path):
    case = case_of(case.tile, case.name)
    masks = list(case.masks.values())
    tune = dict(path.tune)
    pxt = tune.get("pxt_compact", 8)
    assert 256 * pxt == case.tile or tune.get("onepass_form") in FORMS_4096
    ctx = ctx_for(path.algo, path.exp, path.tune, path.vec)
    ctx.set_border(case.border)
    what = f"{case} {path.name}"
    if path.batch != "own":
        # the case's frames repeated up to the big-batch rule (>= 4 frames, >= 20,480 tiles) / one frame short of it
        n = -(-BIG_BATCH_TILES // case.tiles) - (path.batch == "below_big")
        data = op.frames_for(masks, case.h, case.w, case.border, path.dtype, path.kind, 5)
        pick = [i % len(masks) for i in range(n)]
        disp = torch.from_numpy(np.stack(data.frames))[pick].cuda()
        valid = torch.from_numpy(np.stack(masks))[pick].cuda()
        served, spxt, tiles = route(path.algo, case.roi_n, n, pxt, cu=cu_count())
        assert (served == 2) == (path.batch == "big"), (served, n)
        ctx.set_min_disparity(data.dmin)
        device_check(ctx, disp, valid, case.border, path.idx, served, tiles, dmin=data.dmin, what=what)
        return
    data = op.frames_for(masks, case.h, case.w, case.border, path.dtype, path.kind, 5)
    served, _, tiles = route(path.algo, case.roi_n, len(masks), pxt, tune.get("resident_pxt", 0), tune.get("onepass_form", 0), cu_count())
    assert served == (path.algo or 3), (what, served)   # the patterns' batches fit the resident blocks of an MI355X: 0 -> 3 too
    if path.oracle:
        ctx.set_reproject_form(d2pc.FORM_CV24)
    st0 = ctx.compact_stats()
    first = check_compact_is_filtered_parity(ctx, served, data.frames, data.dmin, path.idx, what, scale=data.scale, decoded=data.decoded)
    assert_counters(st0, ctx.compact_stats(), served, tiles, 1, what)   # (for every algorithm: no give-up, no two-pass rerun)
    pts, idx, counts = first
    pix = op.roi_pixels(case.h, case.w, case.border)
    for f, m in enumerate(masks):   # the expected order from the mask itself, never from device output
        assert counts[f] == m.sum(), f"{what} frame {f}: count {counts[f]} != {m.sum()}"
        if path.idx:
            assert np.array_equal(idx[f, :counts[f]], pix[m]), f"{what} frame {f}: idx != pix[valid]"
    second_launch_keeps_the_sentinels(ctx, data, first, path.idx, served, tiles, what)
    if path.oracle:
        q = d2pc.make_q()
        for f, fr in enumerate(data.frames):
            wp, wi = oracle.reproject_compact(fr, q, border=case.border, form=oracle.FORM_CV24, min_disparity=data.dmin)
            assert counts[f] == len(wi) and np.array_equal(idx[f, :len(wi)], wi), f"{what} frame {f}: against the oracle"
            assert np.array_equal(pts[f, :len(wi)].view(np.uint32), wp.view(np.uint32)), f"{what} frame {f}: points against the oracle"


# ------------------------------------------------------------------------------------------------------------- the ladder
Rung = namedtuple("Rung", "rung algo frames tune exp")


def ladder_paths():
    out = []
    for name, tiles, _, _, _ in op.ladder_rungs():
        out.append(Rung(name, 1, 1, (), False))
        if tiles in (1025, 8193) and "ragged" not in name:
            out.append(Rung(name, 1, 2, (), False))           # the scan kernel is one block per frame
        out.append(Rung(name, 2, 1, (), False))
        if tiles == 4097:
            out.append(Rung(name, 2, 2, (), False))
        for r in (0, 8, 32, 64):
            out.append(Rung(name, 3, 1, (("resident_pxt", r),) if r else (), False))
        out.append(Rung(name, 0, 1, (), False))
        out.append(Rung(name, 4, 1, (), True))
    return out


LADDER = ladder_paths()
_rung = {}


def rung_on_device(name):
    """The rung's frame and mask on the device, kept until another rung is asked for."""
    if _rung.get("name") != name:
        _rung.clear()
        torch.cuda.empty_cache()
        _, tiles, w, h, roi_n = next(r for r in op.ladder_rungs() if r[0] == name)
        assert d2pc.roi_points(w, h, 0) == roi_n and -(-roi_n // op.LADDER_TILE) == tiles
        valid = torch.from_numpy(op.ladder_mask(name)).cuda()
        i = torch.arange(roi_n, device="cuda")
        vals = 9.0 + (i * 7 % 883).to(torch.float32) * 0.125        # ordinary finite disparities, 9 .. 119.25
        disp = torch.where(valid, vals, torch.zeros_like(vals)).view(h, w)
        _rung.update(name=name, valid=valid, disp=disp, tiles=tiles, w=w, h=h, roi_n=roi_n)
    return _rung


@pytest.mark.parametrize("r", LADDER, ids=[f"{r.rung}-a{r.algo}x{r.frames}" + "".join(f"-{k}{v}" for k, v in r.tune) for r in LADDER])
def test_tile_count_ladder(r):
    """One or two frames (the second is the first again) of 64 .. 8,193 tiles of 2,048 pixels, border 0, occupancy
    tile_ramp: exactly either side of kSelfScanTiles and the resident forms' 1,024-tile rule, of 4,096 tiles (64 groups;
    the chunked two-pass's 512-group trip) and of the scan kernel's 8 tiles per thread.  Where the router turns the
    resident blocks away the counters say what served instead.  The single pass runs every rung, but the second trip
    of prefix_before's loop over the group words (a tile of group 65 or later met with known.groups == 0) is out of its
    reach on the device: see occupancy_patterns.DEVICE_UNREACHABLE_SLIPS."""
    d = rung_on_device(r.rung)
    tune = dict(r.tune)
    ctx = ctx_for(r.algo, r.exp, r.tune)
    ctx.set_border(0)
    served, spxt, tiles = route(r.algo, d["roi_n"], r.frames, 8, tune.get("resident_pxt", 0), 0, cu_count())
    # (1, 2, 4 serve themselves; 0 / 3 on one frame: resident where a shape of <= 1,024 blocks fits, else the two-pass form)
    assert served == route(r.algo, d["roi_n"], r.frames, 8, tune.get("resident_pxt", 0))[0], "the router of an MI355X (256 CUs)"
    assert served == r.algo if r.algo in (1, 2, 4) else served in (1, 3)
    disp = d["disp"][None].expand(r.frames, d["h"], d["w"]).contiguous()
    valid = d["valid"][None].expand(r.frames, d["roi_n"]).contiguous()
    device_check(ctx, disp, valid, 0, True, served, tiles, what=f"{r}")
