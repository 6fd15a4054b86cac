"""The reprojection kernels over the whole float range (tests/disparity_patterns.py), against the exact answers
(tests/exact_reproject.py), the oracle's named forms, and -- for COMPACT -- the same context's own PARITY output
filtered on the host.  Every bound here is derived, none measured; what each pattern reaches is asserted on the CPU
in tests/test_disparity_patterns.py."""
import os
from types import SimpleNamespace

import numpy as np
import pytest

import disparity_patterns as dp
import disparity_to_point_cloud_amd as d2pc
import exact_reproject as ex
import oracle
from helpers import check_compact_is_filtered_parity, line_bits, run_batch, variant_for

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SHAPE_NAMES = list(dp.SHAPES)
ALL = [(n, s) for s in SHAPE_NAMES for n in dp.FLOAT_PATTERNS]
FORMS = {d2pc.FORM_CV24: oracle.FORM_CV24, d2pc.FORM_CV4: oracle.FORM_CV4}

_ctx = {}


def ctx_for(algo=0, mode=d2pc.MODE_PARITY):
    """One context per compaction algorithm (and build) for the whole module; Q and border are set per test, and everything
    else a test may change -- mode, form, hooks, the disparity floor, the callback tunings -- is put back to its default
    here, so that a failing test leaves nothing behind for the next one."""
    key = (algo, variant_for(algo))
    if key not in _ctx:
        _ctx[key] = d2pc.Context(q=d2pc.make_q(), mode=d2pc.MODE_COMPACT, compact_algo=algo, variant=key[1])
    c = _ctx[key]
    c.set_mode(mode)
    c.set_reproject_form(d2pc.FORM_DEFAULT)
    c.set_test_hook("force_general_q", 0)
    c.set_min_disparity(-np.inf)
    for key, default in (("median_algo", 0), ("callback_fused", 1), ("callback_fused_compact", 2)):
        c.set_tuning(key, default)
    return c


@pytest.fixture(scope="module", autouse=True)
def _close_contexts():
    yield
    for c in _ctx.values():
        c.close()
    _ctx.clear()


def setup(ctx, p, q=None):
    ctx.set_q(p.q if q is None else q)
    ctx.set_border(p.border)


def same_bits(got, want, what=""):
    nan = np.isnan(want)
    assert np.array_equal(nan, np.isnan(got)), what + ": NaN positions"
    assert np.array_equal(got.view(np.uint32)[~nan], want.view(np.uint32)[~nan]), what


def host_frames(p):
    """The pattern's frames as the host path gets them: rows on the shape's padded stride."""
    pitch = dp.SHAPES[p.shape][3]
    return [dp.pitched(f, pitch) for f in p.frames]


def line_distance(got, want_bits):
    return np.abs(line_bits(np.ascontiguousarray(got)) - line_bits(want_bits))


def check_against_exact(got, p, f, what):
    """The default form's contract, frame f of pattern p.

    * within 1 ulp of the correctly rounded value wherever an exact answer exists -- on the integer line of float32
      bit patterns, inf being the float after FLT_MAX, so that subnormal results are held to their own (absolute)
      ulp and no relative tolerance is involved;
    * BIT-EQUAL to it wherever the exact quotient lies farther than 2^-45 (relative) from a float32 rounding boundary:
      the default kernel rounds at most four times in double (the fma for W, u + cx, 1 / W, the product;
      d2pc_pixel.hpp), each by at most 2^-53 relative, so its double result is within 2^-51 of the exact quotient and
      its float cast can differ from the exact rounding only inside that distance of a boundary; 2^-45 leaves a
      factor of 64.  (test_bit_equality_mask_leaves_out_at_most_a_thousandth: the mask keeps > 99.9 % of the points.)
      The sign of a zero is part of the bits;
    * where no exact answer exists (d not finite, W == 0): NaN and +-inf positions and every other bit as the
      oracle's FORM_CV24."""
    e = p.exact
    have = e["has_exact"][f]
    want = e["bits"][f]
    assert np.array_equal(got[:, 3].view(np.uint32), want[:, 3]), what + ": pad word"
    g = got[:, :3]
    assert not np.isnan(g[have]).any(), what + ": NaN where an exact answer exists"
    dist = line_distance(g[have], want[have, :3])
    assert dist.max() <= 1, f"{what}: {dist.max()} ulp from the exactly rounded value"
    m = dp.bit_equal_mask(e)[f]
    bad = (g.view(np.uint32)[m] != want[m, :3])
    assert not bad.any(), f"{what}: {bad.sum()} coordinates differ from the exact rounding away from every boundary"
    if (~have).any():
        o = oracle.reproject(np.ascontiguousarray(p.frames[f]), p.q, border=p.border, form=oracle.FORM_CV24)
        same_bits(g[~have], o[~have, :3], what + ": no exact answer, against the oracle")


# ----------------------------------------------------------------------------------------------- PARITY, default form
@pytest.mark.parametrize("name,shape", ALL)
def test_parity_default_form_against_the_exact_answers(name, shape):
    """Context.process (host path, padded rows) and d2pc_process_device: all frames of the pattern in one launch, a
    one-frame pattern together with its three mirror images (compact_frames), the pattern's frame checked against the
    exact answers.  Patterns of DIFFERENT generators in one launch: test_parity_batch_of_different_patterns."""
    p = dp.with_exact(name, shape)
    ctx = ctx_for()
    setup(ctx, p)
    host = [ctx.process(f).copy() for f in host_frames(p)]
    batch = compact_frames(p)
    assert len(batch) >= 4
    pts, _, _, roi_n = run_batch(ctx, batch, want_index=False)
    for f in range(len(p.frames)):
        check_against_exact(host[f], p, f, f"{name}/{shape} frame {f}")
        check_against_exact(pts[f, :roi_n], p, f, f"{name}/{shape} frame {f}, batched launch")
        assert np.array_equal(pts[f, :roi_n].view(np.uint32), host[f].view(np.uint32)), f"batched launch, frame {f}"
    if name == "binade_sweep":   # the FLT_MAX rule holds for FLT_MAX and not for its neighbour
        d = np.concatenate([f[p.border:f.shape[0] - p.border, p.border:f.shape[1] - p.border].reshape(-1) for f in p.frames])
        z = np.concatenate(host)[:, 2]
        assert (d == ex.FLT_MAX).sum() >= 4 and np.all(z[d == ex.FLT_MAX] == 10000.0)
        below = d == np.nextafter(ex.FLT_MAX, np.float32(0))
        assert below.sum() >= 4 and np.all(z[below] != 10000.0) and np.all(z[below] > 0)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_parity_batch_of_different_patterns(shape):
    """One launch of d2pc_process_device whose frames come from different generators: the sweep's frames with the
    overflow-edge frame between them (both are built for the shape's reference rig, so one Q serves the launch), every
    frame against its own exact answers."""
    sweep, edge = dp.with_exact("binade_sweep", shape), dp.with_exact("overflow_edge", shape)
    assert sweep.q.tobytes() == edge.q.tobytes() and sweep.border == edge.border
    order = [(sweep, f) for f in range(len(sweep.frames))]
    order.insert(len(order) // 2, (edge, 0))
    order.append((edge, 0))
    ctx = ctx_for()
    setup(ctx, sweep)
    pts, _, _, roi_n = run_batch(ctx, [p.frames[f] for p, f in order], want_index=False)
    for i, (p, f) in enumerate(order):
        check_against_exact(pts[i, :roi_n], p, f, f"{shape}: launch frame {i} ({p.name} frame {f})")


# ------------------------------------------------------------------------------------------------ PARITY, named forms
@pytest.mark.parametrize("name,shape", ALL)
def test_parity_named_forms_bit_for_bit(name, shape):
    """D2PC_FORM_CV24 / _CV4 on the stereo kinds and through the general kernel: the oracle's form of the same name,
    bit for bit -- these forms round a * d and b + a * d apart, so the cancellation of w_zero_ordinary is where a
    contracted multiply-add would show."""
    p = dp.make(name, shape)
    ctx = ctx_for()
    setup(ctx, p)
    frames = host_frames(p)
    assert list(FORMS.values())[-1] == oracle.FORM_CV4
    for form, oform in FORMS.items():
        want = [oracle.reproject(np.ascontiguousarray(f), p.q, border=p.border, form=oform) for f in frames]
        for general in (0, 1):
            ctx.set_reproject_form(form)
            ctx.set_test_hook("force_general_q", general)
            for f, fr in enumerate(frames):
                same_bits(ctx.process(fr), want[f], f"form {form} general={general} frame {f}")
    # the default form through the general kernel is OpenCV 4's
    ctx.set_reproject_form(d2pc.FORM_DEFAULT)
    ctx.set_test_hook("force_general_q", 1)
    for f, fr in enumerate(frames):
        same_bits(ctx.process(fr), want[f], f"default form, general kernel, frame {f}")   # (want: FORM_CV4's, the last of FORMS)
    ctx.set_test_hook("force_general_q", 0)


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_stereo_kernel_equals_the_fused_general_evaluation_on_the_sweep(shape):
    """test_general_and_stereo_kernels_agree_bitwise's comparison on the sweep frames: the stereo specialisation drops
    only exact products of the fused multiply-add evaluation of a general Q (experiment build)."""
    p = dp.make("binade_sweep", shape)
    with d2pc.Context(q=p.q, border=p.border, variant="exp") as ctx:
        for f, fr in enumerate(host_frames(p)):
            ctx.set_test_hook("force_general_q", 0)
            a = ctx.process(fr).copy()
            ctx.set_test_hook("force_general_q", 1)
            ctx.set_test_hook("general_q_form", 1)
            same_bits(ctx.process(fr), a, f"frame {f}")
            ctx.set_test_hook("general_q_form", 0)


@pytest.fixture(scope="module")
def dense_q(golden_dir):
    return np.load(os.path.join(golden_dir, "reproject_exact.npz"))["B_dense_q__q"]


@pytest.mark.parametrize("name,shape", ALL)
@pytest.mark.parametrize("w_row", ["dense", "zero_band"])
def test_general_kernel_with_a_dense_q(name, shape, w_row, dense_q):
    """B_dense_q's Q, and that Q with the W row [0, 0, a, b] of the pattern's own rig (so that W passes through zero
    and the sliver as it does there), every frame of the pattern: OpenCV 4's form bit for bit, PARITY and COMPACT (the
    context's default routing of the compaction; the algorithms are told apart on the stereo Q, forced through the
    general kernel, in test_compact_equals_the_filtered_parity_output)."""
    p = dp.make(name, shape)
    q = dense_q.copy()
    if w_row == "zero_band":
        q[12:16] = [0.0, 0.0, p.q[14], p.q[15]]
    ctx = ctx_for()
    setup(ctx, p, q)
    for f, fr in enumerate(host_frames(p)):
        same_bits(ctx.process(fr), oracle.reproject(np.ascontiguousarray(fr), q, border=p.border, form=oracle.FORM_CV4), f"frame {f}")
        ctx.set_mode(d2pc.MODE_COMPACT)
        gp, gi = ctx.process(fr, want_index=True)
        wp, wi = oracle.reproject_compact(np.ascontiguousarray(fr), q, border=p.border, form=oracle.FORM_CV4)
        assert np.array_equal(gi, wi)
        same_bits(gp, wp, f"compact, frame {f}")
        ctx.set_mode(d2pc.MODE_PARITY)


# --------------------------------------------------------------------------------------------------- U8 / U16 decode
@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("kind", ["u16", "u8"])
def test_integer_decode_over_every_raw_value(kind, shape):
    """float(raw) * scale in the kernel: bit-identical to feeding raw.astype(float32) * float32(scale) as fp32 -- one
    fp32 rounding, subnormal products kept, overflow to inf -- for all 65,536 / 256 raw values and every scale; against
    the oracle with scale=: the named forms bit for bit; the default form and the oracle's FORM_CV24 are each within 1 ulp of the exact value, so
    within 2 of each other (inf being the float after FLT_MAX), NaN positions identical.  At the two small shapes the
    default form is also held to the exact answers of the decoded frame, for every scale; at the native shape that
    evaluation (268,800 distinct pixels x 5 scales x 2 types) is left out for its run time alone -- the raw values, the
    scales and the kernel's decode are the same there, and the load path plays no part in the arithmetic."""
    p = (dp.u16_all_values if kind == "u16" else dp.u8_all_values)(3, shape)
    raw = host_frames(p)[0]
    ctx = ctx_for()
    setup(ctx, p)
    for scale in p.scales:
        fed = dp.pitched(dp.decode(p.frames[0], scale), dp.SHAPES[shape][3])
        for form in (d2pc.FORM_DEFAULT, d2pc.FORM_CV24, d2pc.FORM_CV4):
            ctx.set_reproject_form(form)
            got = ctx.process(raw, scale=scale).copy()
            assert np.array_equal(got.view(np.uint32), ctx.process(fed).view(np.uint32)), f"scale {scale}, form {form}"
            want = oracle.reproject(np.ascontiguousarray(raw), p.q, border=p.border, scale=scale, form=FORMS.get(form, oracle.FORM_CV24))
            if form == d2pc.FORM_DEFAULT:
                nan = np.isnan(want)
                assert np.array_equal(nan, np.isnan(got)), f"scale {scale}"
                ok = ~nan[:, :3]
                assert line_distance(got[:, :3][ok], want[:, :3].view(np.uint32)[ok]).max() <= 2, f"scale {scale}"
            else:
                same_bits(got, want, f"scale {scale}, form {form}")
        ctx.set_reproject_form(d2pc.FORM_DEFAULT)
    if shape != "native":   # ... and the default form against the exact answers of the decoded frame
        for scale in p.scales:
            fed_p = SimpleNamespace(q=p.q, border=p.border, frames=dp.decode(p.frames, scale), shape=shape)
            fed_p.exact = ex.exact_reproject(fed_p.q, fed_p.frames, fed_p.border)
            check_against_exact(ctx.process(raw, scale=scale), fed_p, 0, f"{kind} scale {scale}")


# ------------------------------------------------------------------------------------------ COMPACT, every algorithm
def floors_of(p):
    """Disparity floors: off, a value that occurs in the pattern's frames, and its two float neighbours."""
    pool = np.unique(p.frames[np.isfinite(p.frames) & (p.frames > 0)])
    v = np.float32(pool[len(pool) // 2])
    return [float(np.nextafter(v, np.float32(-np.inf))), float(v), float(np.nextafter(v, np.float32(np.inf)))]


def compact_frames(p):
    """At least four frames per launch, so that the single pass and the resident blocks serve a real batch: a
    one-frame pattern is joined by its mirror images."""
    fr = list(p.frames)
    if len(fr) == 1:
        fr += [np.ascontiguousarray(fr[0][::-1]), np.ascontiguousarray(fr[0][:, ::-1]), np.ascontiguousarray(fr[0][::-1, ::-1])]
    return fr


@pytest.mark.parametrize("name,shape", ALL)
@pytest.mark.parametrize("algo", [1, 2, 3, 4])
def test_compact_equals_the_filtered_parity_output(name, shape, algo):
    """Every compaction algorithm on every pattern and shape, with a SAMPLE of ten of the (form, kernel, floor, index)
    combinations (`cases`: each form, the general kernel in two forms, with and without indices, the floor off / on a
    value of the frame / on its float neighbours) -- the matrix is thinned, the values are not.  On w_zero_sliver
    and overflow_edge cheap-predicate and exact-path pixels alternate inside one tile.  Every frame also against
    oracle.reproject_compact where the form is a named one."""
    p = dp.make(name, shape)
    frames = compact_frames(p)
    ctx = ctx_for(algo)
    setup(ctx, p)
    lo, at, hi = floors_of(p)
    cases = [(d2pc.FORM_DEFAULT, 0, -np.inf, True), (d2pc.FORM_DEFAULT, 0, -np.inf, False), (d2pc.FORM_CV24, 0, -np.inf, True),
             (d2pc.FORM_CV4, 0, -np.inf, True), (d2pc.FORM_DEFAULT, 1, -np.inf, True), (d2pc.FORM_CV24, 1, -np.inf, False),
             (d2pc.FORM_DEFAULT, 0, at, True), (d2pc.FORM_DEFAULT, 0, lo, True), (d2pc.FORM_DEFAULT, 0, hi, False),
             (d2pc.FORM_CV4, 0, at, True)]
    for form, general, dmin, want_index in cases:
        ctx.set_reproject_form(form)
        ctx.set_test_hook("force_general_q", general)
        what = f"algo {algo} form {form} general={general} floor {dmin}"
        pts, idx, counts = check_compact_is_filtered_parity(ctx, algo, frames, dmin, want_index, what)
        oform = FORMS.get(form) if form in FORMS else (oracle.FORM_CV4 if general else None)
        if oform is not None and want_index:   # ... and the oracle's compaction in the named forms
            for f, fr in enumerate(frames):
                wp, wi = oracle.reproject_compact(fr, p.q, border=p.border, form=oform, min_disparity=dmin)
                assert counts[f] == len(wi) and np.array_equal(idx[f, :len(wi)], wi), f"{what} frame {f}"
                same_bits(pts[f, :len(wi)], wp, f"{what} frame {f}: against the oracle")


@pytest.mark.parametrize("shape", SHAPE_NAMES)
@pytest.mark.parametrize("algo", [1, 2, 3, 4])
def test_compact_of_16_bit_input(shape, algo):
    """U16 frames through every algorithm with the scales that make small raw values subnormal and large ones inf."""
    p = dp.u16_all_values(3, shape)
    frames = compact_frames(p)
    ctx = ctx_for(algo)
    setup(ctx, p)
    for scale in (p.scales[0], p.scales[3], p.scales[4]):
        decoded = [dp.decode(f, scale) for f in frames]
        fin = np.sort(decoded[0][np.isfinite(decoded[0])])
        dmin = float(fin[len(fin) // 2])
        for floor in (-np.inf, dmin):
            check_compact_is_filtered_parity(ctx, algo, frames, floor, True, f"algo {algo} scale {scale} floor {floor}", scale=scale, decoded=decoded)


# ------------------------------------------------------------------------------------------- the fused callback body
def _mono(ctx, b, src, w, h, n, k, scale, key, fused):
    ctx.set_tuning(key, fused)
    b.points.fill_(0)
    b.index.fill_(-1)
    b.counts.fill_(-7)
    ctx.process_mono_device(src.data_ptr(), d2pc.DTYPE_U8, w, h, w, w * h, n, k, scale, b.points.data_ptr(),
                            b.index.data_ptr(), b.stride, b.counts.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ctx.check_async_error()
    return (b.points.cpu().numpy().view(np.uint32).copy(), b.index.cpu().numpy().view(np.uint32).copy(),
            b.counts.cpu().numpy().view(np.uint32).copy())


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT])
@pytest.mark.parametrize("k", [0, 3])
def test_callback_body_tables_over_every_byte_and_scale(k, mode):
    """d2pc_process_mono_device on frames that hold every byte -- unfiltered (k = 0) and as 3 x 3 constant cells through the
    3 x 3 median, which is the identity at the cell centres -- with scales that straddle subnormal and overflow: the
    tile-fused kernels (per-block 256-entry tables of 1 / W, Z and validity, d2pc_callback.hip) against the two
    launches, and both against the plain U8 reprojection of the filtered frame, bit for bit.  At the native shape only
    (four frames, so that the one-kernel form serves the launch): the tables are indexed by the byte, not by the geometry."""
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch
    w, h, border, _ = dp.SHAPES["native"]
    n = 4   # 528 tiles: the one-kernel form serves the launch
    rng = np.random.default_rng(41)
    if k:
        imgs = [dp.constant_cells(rng, h, w, border, k) for _ in range(n)]
        frames = [i for i, _ in imgs]
        filt = [oracle.median_u8(f, k) for f in frames]
        for (img, centre), m in zip(imgs, filt):
            assert np.array_equal(m[centre], img[centre]) and len(np.unique(img[centre])) == 256
    else:
        frames = [dp.u8_all_values(s, "native").frames[0] for s in range(n)]
        filt = frames
    compact = mode == d2pc.MODE_COMPACT
    key, forms = ("callback_fused_compact", (2, 1, 0)) if compact else ("callback_fused", (1, 0))
    ctx = ctx_for(0, mode)
    ctx.set_q(d2pc.make_q())
    ctx.set_border(border)
    ctx.set_tuning("median_algo", 2)
    src = torch.from_numpy(np.stack(frames)).cuda()
    b = DeviceBatch(ctx, n, h, w, dtype=torch.uint8, want_index=True)
    for scale in dp.U8_SCALES:
        res = {fused: _mono(ctx, b, src, w, h, n, k, scale, key, fused) for fused in forms}
        for fused in forms[:-1]:
            for x, y in zip(res[fused], res[forms[-1]]):
                assert np.array_equal(x, y), f"scale {scale}: form {fused} differs from the two launches"
        pts, idx, cnt, _ = run_batch(ctx, filt, want_index=True, scale=scale)   # the plain U8 path on the filtered frames
        assert np.array_equal(res[forms[0]][2], cnt), f"scale {scale}: counts"
        for f in range(n):
            c = int(cnt[f])
            assert np.array_equal(res[forms[0]][0][f, :c], pts[f, :c].view(np.uint32)), f"scale {scale}, frame {f}: points"
            assert np.array_equal(res[forms[0]][1][f, :c], idx[f, :c]), f"scale {scale}, frame {f}: indices"
