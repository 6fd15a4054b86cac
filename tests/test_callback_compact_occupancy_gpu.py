"""The fused COMPACT callback kernels on built occupancy patterns (tests/callback_patterns.py), above all the pipelined
one (k_callback_bs_compact_pipe, `callback_fused_compact` 2) in its STEADY STATE: a block that walks several tiles,
keeps tile i - 1's filtered bytes while it filters tile i, asks early for the words that place tile i - 1
(CbEarlyPlace::request) and reads them behind the count (take).

Routing.  d2pc_process_mono_device gives every frame per_frame = min(resident / n, tiles_per_frame) blocks, resident =
cu_count * min(callback_pipe_blocks_per_cu, 3).  With the default 3 per CU every small batch gets one block per tile,
and then no block ever holds a previous and a current tile together.  The steady-state cases set
`callback_pipe_blocks_per_cu` to 1 -- fewer persistent blocks than the device admits, never more -- and take n from
the device's CU count so that tiles_x < per_frame < tiles_per_frame (`route`, asserted per case): some block holds two
tiles or more.  On 256 CUs:

  shape      ROI          tiles    n   per_frame
  five       1031 x 250   5 x 8    16  16     ragged in x and y; five_odd (1031 x 249): the last row pair is half outside
  five_min   1031 x 250   5 x 8    42  6      per_frame = tiles_x + 1, the least the no-deadlock argument allows
  sixteen    4096 x 96    16 x 3   8   32     the early look's four row words per lane just fit
  seventeen  4097 x 96    17 x 3   8   32     they do not: the tile is placed by cb_look
  tall       256 x 4160   1 x 130  8   32     bands above pass 64 / 65: take() reads band[1]; tall2: 257 wide, 2 x 130
  taller     256 x 6400   1 x 200  8   32     bands above pass 128 / 129 in tiles the early look is asked for: `fits` false;
                                              taller2: 257 wide, 2 x 200
  small3     672 x 400    3 x 13   3   39     default residency: one tile per block, the routing the suite already uses

Which tiles the steady state places.  A block draws the ticket behind tile T when it starts to filter T, and T goes through
request / take only if that ticket is still below tiles_per_frame; otherwise the block has no tile to filter while T
waits, and T is placed by cb_look as in the one-tile-per-block form.  Between two draws of a block every other block of
the frame draws about once, so the ticket behind T is about T + per_frame: roughly the first tiles_per_frame - per_frame
tiles of a frame take the early look, and each block's last tile never does -- on `sixteen` the 16 tiles of band 0 (nothing
above them), on `seventeen` about 19 tiles, on `five` about 24 of 40, on `five_min` about 34.  On `tall` the one tile with
more than 128 bands above is the frame's last ticket, and on `tall2` the two last: they are placed by cb_look, and `fits`
false for the band words (ty > 128) is NOT reached there.  `taller` / `taller2` are high enough that the tiles of band 129
lie more than 2 * per_frame tickets before the frame's end (`assert_early_look_meets_band_129`): with
that margin they are asked for early, find `fits` false and fall back to cb_look from inside the steady state.  Which block
draws which ticket is the dispatcher's affair, so this is a margin, not a proof; when written, a scratch build whose `fits`
admitted ty = 129 with the 128 band words it has failed exactly the 16 `taller` / `taller2` cases and no `tall` one.

Holes.  The kind of hole follows (general_q + (k == 11)) % 2: every (routing, generator, k) meets zeros and floor bytes, but
under one kernel each -- k = 3 zeros under the stereo kernel and floor bytes under the general one, k = 11 the other way
round -- never the same kind under both; that halves the run time.

Per case: forms 2, 1 and 0 on one context, each launched twice into buffers of sentinel bits (points: a NaN payload,
indices: a value beyond the batch).  Points (as bits), indices and counts of the three forms are equal; the second
launch equals the first; nothing from `count` to the stride is written; indices equal pix[np.flatnonzero(valid)] and
counts valid.sum() from the oracle's median; frame 0's points against oracle.reproject_compact (FORM_CV4 at 0 ulp under
force_general_q, the default form within 1 ulp); spin_timeout_ms 500, no time-out, no count of 0xFFFFFFFF, no
asynchronous error; the fused forms count one state clear per sub-batch (`launches`), which is asserted against the
restated router.  What every case's input reaches, and that the numpy model kills each of its slips on these cases, is
asserted without a GPU in tests/test_callback_patterns.py, which imports `CASES` from here; `case_of` refuses others."""
from collections import namedtuple

import numpy as np
import pytest

import callback_patterns as cp
import disparity_to_point_cloud_amd as d2pc
import oracle
from helpers import assert_points_close
from route_model import CU_DEFAULT, PIPE_BLOCKS_PER_CU_DEFAULT, callback_route

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

PT_SENTINEL, IX_SENTINEL = 0x7FC5A5A5, 0x5A5AA5A5   # a NaN with a payload no kernel produces; an index beyond any batch here
# Scales at which every non-zero byte decodes to a sliver W (table class 2: a block then takes the exact path for good).
# 1.3e-41 is the degenerate-scale test's: Z = f / W overflows for every byte, nothing survives.  At 3e-39 W = q32 * d lies
# below w_safe (about 735 * 2^-126 = 8.6e-36) for every byte as well, but from byte 63 or so on Z = f / W is finite: whether a
# pixel survives depends on the VALUE of the filtered byte, which the tables' classes cannot tell.
SLIVER_SCALES = (1.3e-41, 3e-39)

# name -> (shape of callback_patterns.SHAPES, blocks per CU, the per_frame the frame count aims at; 0: n = 3)
ROUTINGS = {"five": ("five", 1, 16), "five_odd": ("five_odd", 1, 16), "five_min": ("five", 1, 6), "sixteen": ("sixteen", 1, 32),
            "seventeen": ("seventeen", 1, 32), "tall": ("tall", 1, 32), "tall2": ("tall2", 1, 32),
            "taller": ("taller", 1, 32), "taller2": ("taller2", 1, 32),
            "small3": ("small3", PIPE_BLOCKS_PER_CU_DEFAULT, 0)}
STEADY = tuple(r for r in ROUTINGS if r != "small3")
BAND_129 = ("taller", "taller2")      # the early look is asked for tiles with more than 128 bands above
EARLY_LOOK_BANDS = 128
GENERATORS_ON = {"five": cp.GENERATORS, "five_odd": ("row_counts", "edges"), "five_min": ("tile_ramp", "row_counts"),
                 "sixteen": ("tile_ramp", "tile_steps"), "seventeen": ("tile_ramp", "tile_steps"),
                 "tall": ("tile_ramp", "empty_bands"), "tall2": ("tile_ramp", "empty_bands"),
                 "taller": ("tile_ramp", "empty_bands"), "taller2": ("tile_ramp", "empty_bands"), "small3": ("row_counts", "edges")}

Case = namedtuple("Case", "routing generator k general_q holes scale part")


def case_id(c):
    return f"{c.routing}-{c.generator}{'' if c.part is None else c.part}-k{c.k}-gq{c.general_q}-{c.holes}" + \
           (f"-scale{c.scale:g}" if c.scale != cp.SCALE else "")


def _cases():
    out = []
    for routing, gens in GENERATORS_ON.items():
        for gen in gens:
            for k in (3, 11):
                for gq in (0, 1):
                    holes = cp.HOLES[(gq + (k == 11)) % 2]      # both kinds of hole for every (generator, k)
                    # (three frames per launch on small3: the seven frames of `edges` go in three parts)
                    parts = (0, 1, 2) if (routing, gen) == ("small3", "edges") else (None,)
                    out += [Case(routing, gen, k, gq, holes, cp.SCALE, p) for p in parts]
    out += [Case("five", "row_counts", 11, 0, "zero", s, None) for s in SLIVER_SCALES]
    return out


CASES = _cases()
SMALL3_EDGE_PARTS = (("cols", "first_row", "last_row"), ("first_px", "none", "full"), ("full", "none", "last_px"))


def case_of(cid):
    """Only the cases whose reach tests/test_callback_patterns.py asserts are run."""
    for c in CASES:
        if case_id(c) == cid:
            return c
    raise AssertionError(f"{cid} is not a case of CASES: its reach is asserted nowhere")


def pattern_of(case):
    return cp.pattern(case.generator, ROUTINGS[case.routing][0], case.k, case.holes)


def frame_order(case, n):
    """-> which of the pattern's frames stands at each of the n places of the batch."""
    p = pattern_of(case)
    if case.part is not None:
        return [p.names.index(x) for x in SMALL3_EDGE_PARTS[case.part]]
    return [f % len(p.frames) for f in range(n)]


# ----------------------------------------------------------------------------------------- the router, restated in route_model
def route(routing, cu=CU_DEFAULT):
    """The residency rule for the fused COMPACT forms (route_model.callback_route) on a routing of ROUTINGS: -> Route."""
    shape, per_cu, aim = ROUTINGS[routing]
    return callback_route(*cp.SHAPES[shape], per_cu, aim, cu)


def assert_steady(r, what):
    """Fewer blocks than tiles per frame, in one sub-batch, served by the pipelined kernel: some block walks tiles."""
    assert r.n >= 1 and r.n <= r.nfc and r.sub_batches == 1, (what, r)
    assert r.tiles_x < r.per_frame < r.tpf and r.pipelined, (what, r)
    assert r.per_frame * r.n < r.tpf * r.n


def assert_early_look_meets_band_129(r, what):
    """The first tile with more than 128 bands above it has ticket 129 * tiles_x.  It takes the early look if the ticket its
    block draws while filtering it is a tile's: with every block drawing about once in between that is ticket + per_frame,
    and twice that is required to lie inside the frame."""
    assert r.tiles_y > EARLY_LOOK_BANDS + 1 and (EARLY_LOOK_BANDS + 1) * r.tiles_x + 2 * r.per_frame < r.tpf, (what, r)


# --------------------------------------------------------------------------------------------------------------- contexts
_ctx = {}


def ctx_for(case):
    b = cp.BORDER[case.k]
    if b not in _ctx:
        _ctx[b] = d2pc.Context(q=d2pc.make_q(), border=b, mode=d2pc.MODE_COMPACT)
    c = _ctx[b]
    c.set_test_hook("force_general_q", case.general_q)
    c.set_reproject_form(d2pc.FORM_DEFAULT)
    c.set_min_disparity(cp.dmin_of(case.holes))
    c.set_tuning("median_algo", 2)
    c.set_tuning("spin_timeout_ms", 500)
    c.set_tuning("callback_pipe_blocks_per_cu", ROUTINGS[case.routing][1])
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    torch.cuda.reset_peak_memory_stats()
    _used.clear()
    _used.append(device_bytes_in_use())
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()
    torch.cuda.empty_cache()
    # torch's figure covers torch's allocator only; the contexts' own state and scratch buffers (hipMalloc) show in the
    # device-wide figure, sampled behind every case's launches (it also holds what torch caches and what others use)
    print("\npeak device memory of test_callback_compact_occupancy_gpu.py: %.3f GiB in torch's allocator; device-wide in use "
          "%.3f GiB at the start, at most %.3f GiB behind a case" % (torch.cuda.max_memory_allocated() / 2**30, _used[0] / 2**30,
                                                                    max(_used) / 2**30))


_used = []


def device_bytes_in_use():
    free, total = torch.cuda.mem_get_info()
    return total - free


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


def launch_forms(ctx, src, k, scale, n, h, w, sub_batches, what):
    """Forms 2, 1, 0, each twice into sentinel-filled buffers -> {form: (points as int32, indices, counts)} of the first
    launches, on the device; the hand-off checks and the tail of every launch are asserted here."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
    s = torch.cuda.current_stream().cuda_stream
    pts = b.points.view(torch.int32)
    beyond = torch.arange(b.stride, device="cuda")[None, :]
    res = {}
    for form in (2, 1, 0):
        ctx.set_tuning("callback_fused_compact", form)
        for launch in range(2):
            pts.fill_(PT_SENTINEL)
            b.index.fill_(IX_SENTINEL)
            b.counts.fill_(-7)
            st0 = ctx.compact_stats()
            ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, k, scale, b.points.data_ptr(),
                                    b.index.data_ptr(), b.stride, b.counts.data_ptr(), s)
            torch.cuda.synchronize()
            ctx.check_async_error()
            st = ctx.compact_stats()
            tag = f"{what}, form {form}, launch {launch}"
            assert st["timeouts"] == st0["timeouts"] == 0, (tag, st)
            if form:     # launch_state_clear counts a launch per sub-batch of the fused forms
                assert st["launches"] == st0["launches"] + sub_batches, (tag, st0, st)
            counts = b.counts.to(torch.int64) & 0xFFFFFFFF
            assert not bool((counts == 0xFFFFFFFF).any()), f"{tag}: a frame reports a timed-out hand-off"
            assert bool((counts <= b.roi_n).all()), tag
            tail = beyond >= counts[:, None]
            assert bool((pts[tail] == PT_SENTINEL).all()), f"{tag}: points written at or beyond count"
            assert bool((b.index[tail] == IX_SENTINEL).all()), f"{tag}: indices written at or beyond count"
            if launch == 0:
                res[form] = (pts.clone(), b.index.clone(), counts.clone())
            else:
                for first, again, name in zip(res[form], (pts, b.index, counts), ("points", "indices", "counts")):
                    assert torch.equal(first, again), f"{tag}: {name} differ from the first launch"
    _used.append(device_bytes_in_use())
    for form in (2, 1):
        for got, ref, name in zip(res[form], res[0], ("points", "indices", "counts")):
            assert torch.equal(got, ref), f"{what}: {name} of form {form} differ from the two launches"
    return res, b.stride


@pytest.mark.parametrize("cid", [case_id(c) for c in CASES])
def test_callback_compact_on_built_occupancy(cid):
    """One case of `CASES` (see the module's docstring): the routing asserted from the device's CU count, forms 2, 1, 0 twice
    each, then the oracle's median for indices and counts and the oracle's compaction for frame 0's points."""
    case = case_of(cid)
    r = route(case.routing, cu_count())
    if case.routing in STEADY:
        assert_steady(r, cid)
        if case.routing in BAND_129:
            assert_early_look_meets_band_129(r, cid)
    else:
        assert r.per_frame == r.tpf and r.sub_batches == 1, r      # one tile per block
    p = pattern_of(case)
    order = frame_order(case, r.n)
    src = torch.from_numpy(np.stack([p.frames[i] for i in order])).cuda()
    ctx = ctx_for(case)
    res, stride = launch_forms(ctx, src, case.k, case.scale, r.n, p.h, p.w, r.sub_batches, cid)
    if case.scale != cp.SCALE:
        # a sliver scale: validity is the arithmetic's, and the two launches are the reference
        total, most = int(res[0][2].sum()), sum(int(p.valid[i].sum()) for i in order)
        assert total == 0 if case.scale == SLIVER_SCALES[0] else 0 < total < most, (cid, total, most)
        return
    pts, idx, counts = res[2]
    pix = p.pix()
    want_idx = np.full((len(p.frames), stride), IX_SENTINEL, dtype=np.int64)
    want_n = np.zeros(len(p.frames), dtype=np.int64)
    for i in set(order):
        wi = pix[np.flatnonzero(p.valid[i])]
        want_idx[i, :len(wi)], want_n[i] = wi, len(wi)
    assert np.array_equal(counts.cpu().numpy(), want_n[order]), (cid, counts.cpu().numpy(), want_n[order])
    got_idx = idx.cpu().numpy().view(np.uint32)
    for f, i in enumerate(order):
        assert np.array_equal(got_idx[f], want_idx[i]), f"{cid}: indices of frame {f} ({p.names[i]})"
    # frame 0 against the oracle's compaction of the oracle's median
    form, ulp = (oracle.FORM_CV4, 0) if case.general_q else (oracle.FORM_CV24, 1)
    want, wi = oracle.reproject_compact(p.medians[order[0]], d2pc.make_q(), border=p.border, scale=case.scale, form=form,
                                        min_disparity=p.dmin)
    assert len(want) == want_n[order[0]] and np.array_equal(wi, want_idx[order[0], :len(wi)])
    if len(want):
        got = pts[0, :len(want)].cpu().numpy().view(np.float32)
        assert_points_close(got, want, max_ulp=ulp, rel=1e-5, what=f"{cid} frame 0")


def test_residency_tuning_cuts_the_batch_where_the_restated_router_does():
    """One frame more than `nfc` under callback_pipe_blocks_per_cu 1 makes two sub-batches, where the default residency
    makes one: the `launches` counter shows that the tuning the steady-state cases rely on took hold."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    case = case_of("five_min-tile_ramp-k3-gq0-zero")
    cu = cu_count()
    r = route("five_min", cu)
    n = r.nfc + 1
    assert n <= 3 * cu // (r.tiles_x + 1)
    p = pattern_of(case)
    src = torch.from_numpy(np.stack([p.frames[0]] * n)).cuda()
    ctx = ctx_for(case)
    ctx.set_tuning("callback_fused_compact", 2)
    b = DeviceBatch(ctx, n, p.h, p.w, dtype=torch.uint8, want_index=True)
    want = pattern_of(case).pix()[np.flatnonzero(p.valid[0])]
    for per_cu, subs in ((1, 2), (PIPE_BLOCKS_PER_CU_DEFAULT, 1)):
        ctx.set_tuning("callback_pipe_blocks_per_cu", per_cu)
        b.index.fill_(IX_SENTINEL)
        b.counts.fill_(-7)
        st0 = ctx.compact_stats()
        ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, p.w, p.h, p.w, p.w * p.h, n, case.k, case.scale, b.points.data_ptr(),
                                b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        ctx.check_async_error()
        st = ctx.compact_stats()
        assert st["timeouts"] == 0 and st["launches"] == st0["launches"] + subs, (per_cu, st0, st)
        assert bool((b.counts == len(want)).all())
        idx = b.index.cpu().numpy().view(np.uint32)
        assert all(np.array_equal(idx[f, :len(want)], want) for f in (0, r.nfc - 1, r.nfc))
