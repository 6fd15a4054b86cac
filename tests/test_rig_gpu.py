"""The rig session (d2pc_rig_*): n cameras of one geometry, each with its own Q, one merged cloud per call.

Expected answers come from two independent sources: the oracle, called per camera with that camera's Q and
concatenated, and the library's own d2pc_process_device on that camera's frame alone after d2pc_set_q(Q_f).  The
tolerances are the project's: under FORM_CV4 0 ulp from the oracle's CV4 form for every Q; under the default form <= 1
ulp from the oracle for stereoRectify Qs and 0 ulp for dense (posed) ones; the bytes of d2pc_process_device in both
forms; counts, offsets and indices exact.  Outputs are pre-filled with sentinel bits, and every word past the cloud
must still hold them.

With holes written as d = 0, NaN, inf or a value at the disparity floor, the survivors of every camera are exactly the
mask's pixels whatever its pose (a T whose last row is 0 0 0 1 leaves W untouched): np.flatnonzero(valid) is the
expected order, and tests/occupancy_patterns.py's masks are used unchanged."""
import math
from types import SimpleNamespace

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import occupancy_patterns as op
import oracle
from disparity_to_point_cloud_amd import capi
from helpers import assert_points_close, run_batch

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
PT_SENTINEL, IX_SENTINEL = 0x7FC5A5A5, 0x5A5AA5A5   # a NaN with a payload no kernel produces; an index beyond any batch
GUARD = 96                                         # sentinel words kept past every output
COMPACT_TILE, SCAN_TRIP = 1024, 4096               # d2pc_rig.hpp: pixels per COMPACT tile, tiles per trip of the scan
INVALID_ARG, BAD_SIZE, CAPACITY = 1, 3, 4
DTC = {"f32": d2pc.DTYPE_F32, "u8": d2pc.DTYPE_U8, "u16": d2pc.DTYPE_U16}
SHAPES = {"three": (3, 37, 70, 3),   # ROI 64 x 31 = 1,984 points: ragged tiles, camera starts off 128-byte alignment
          "five": (5, 12, 20, 2)}    # ROI 16 x 8 = 128 points: less than a tile per camera


def pose_q(q):
    """A camera turned 72 degrees about y and moved: T.Q, dense."""
    a = math.radians(72.0)
    t = np.array([[math.cos(a), 0, math.sin(a), 0.35], [0, 1, 0, -0.12], [-math.sin(a), 0, math.cos(a), 0.08], [0, 0, 0, 1.0]])
    return d2pc.rig_compose_q(t, q).reshape(16)


def rig_qs(n):
    """(Q, is it stereoRectify's) per camera: the default, other intrinsics, posed; then the identity-composed default
    (still stereoRectify's structure) and a posed camera with the other intrinsics."""
    q0 = d2pc.make_q()
    q1 = d2pc.make_q(fx=601.5, fy=598.25, cx=331.75, cy=233.5, baseline=0.12, nx=640, ny=480)
    qs = [(q0, True), (q1, True), (pose_q(q0), False), (d2pc.rig_compose_q(np.eye(4), q0).reshape(16), True), (pose_q(q1), False)]
    return qs[:n] if n <= 5 else [qs[i % 5] for i in range(n)]


@pytest.fixture(scope="module")
def ctxs():
    """(the rig's context, the context of the per-camera reference calls)."""
    with d2pc.Context(q=d2pc.make_q(), border=3) as a, d2pc.Context(q=d2pc.make_q(), border=3, compact_algo=1) as b:
        yield a, b


def configure(ctxs, border, mode, form=d2pc.FORM_DEFAULT, dmin=-np.inf):
    for c in ctxs:
        c.set_border(border)
        c.set_mode(mode)
        c.set_reproject_form(form)
        c.set_min_disparity(dmin)


def to_device(frames, pad):
    """frames: list of (h, w) numpy -> (backing tensor, pointer, row stride, frame stride); pad: rows 24 bytes longer,
    frames 3 rows further apart than they need to be."""
    stack = np.stack(frames)
    n, h, w = stack.shape
    es = stack.itemsize
    pitch = w * es + (24 if pad else 0)
    fstride = (h + (3 if pad else 0)) * pitch
    buf = torch.full((n * fstride + 64,), 0x3C, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((n, h, w * es), (fstride, pitch, 1), 0)
    view.copy_(torch.from_numpy(stack.view(np.uint8).reshape(n, h, w * es)).to(DEV))
    return buf, buf.data_ptr(), pitch, fstride


def run_rig(rig, frames, scale, want_index, pad=False, capacity=None, stream=None):
    """One call into sentinel-filled buffers -> SimpleNamespace(points, index, counts, offsets) as numpy, whole buffers."""
    n = len(frames)
    cap = int(rig.geometry().capacity_points) if capacity is None else capacity
    keep = to_device(frames, pad)
    pts = torch.full(((cap + GUARD) * 4,), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((cap + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV) if want_index else None
    counts = torch.full((n + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    offsets = torch.full((n + 1 + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    rig.process_device(keep[1], scale, keep[2], keep[3], pts.data_ptr(), idx.data_ptr() if want_index else None, cap,
                       counts.data_ptr(), offsets.data_ptr(), stream if stream is not None else torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    rig.ctx.check_async_error()
    u32 = lambda t: t.cpu().numpy().view(np.uint32)  # noqa: E731
    return SimpleNamespace(points=u32(pts).reshape(-1, 4), index=u32(idx) if want_index else None, counts=u32(counts),
                           offsets=u32(offsets), cap=cap)


def check_cloud(got, ctxs, frames, qs, scale, border, compact, form, dmin, want_index, what, valid=None):
    """The merged cloud against the oracle and against d2pc_process_device, camera by camera; counts, offsets, indices and
    the sentinels past the cloud."""
    ref = ctxs[1]
    n, (h, w) = len(frames), frames[0].shape
    pix = op.roi_pixels(h, w, border)
    assert np.all(got.counts[n:] == IX_SENTINEL) and np.all(got.offsets[n + 1:] == IX_SENTINEL), what
    assert got.offsets[0] == 0 and np.array_equal(np.diff(got.offsets[:n + 1].astype(np.int64)), got.counts[:n]), what
    total = int(got.offsets[n])
    for f, (fr, (q, stereo)) in enumerate(zip(frames, qs)):
        a, c = int(got.offsets[f]), int(got.counts[f])
        mine = got.points[a:a + c]
        ref.set_q(q)
        rp, ri, rc, roi_n = run_batch(ref, [fr], want_index=True, scale=scale)
        if compact:
            wp, wi = oracle.reproject_compact(fr, q, border=border, scale=scale, form=oracle.FORM_CV4, min_disparity=dmin)
            if valid is not None:
                assert np.array_equal(wi, pix[np.flatnonzero(valid[f])]), f"{what} camera {f}: the oracle's survivors are not the mask's"
        else:
            wp, wi = oracle.reproject(fr, q, border=border, scale=scale, form=oracle.FORM_CV4), pix
        assert c == len(wp) == int(rc[0]), f"{what} camera {f}: count {c}, oracle {len(wp)}, process_device {rc[0]}"
        exact = form == d2pc.FORM_CV4 or not stereo
        assert_points_close(mine.view(np.float32), wp, max_ulp=0 if exact else 1, what=f"{what} camera {f} vs oracle")
        assert np.array_equal(mine, rp[0, :c].view(np.uint32)), f"{what} camera {f}: bytes differ from d2pc_process_device"
        if want_index:
            assert np.array_equal(got.index[a:a + c].astype(np.int64) - f * w * h, wi), f"{what} camera {f}: indices"
            assert np.array_equal(ri[0, :c], wi)
    assert np.all(got.points[total:] == PT_SENTINEL), f"{what}: a point past the cloud was written"
    if want_index:
        assert np.all(got.index[total:] == IX_SENTINEL), f"{what}: an index past the cloud was written"
    return total


def random_frames(n, h, w, dtype, seed):
    """Ordinary finite disparities everywhere."""
    return op.frames_for([np.ones(h * w, dtype=bool)] * n, h, w, 0, dtype, "zero", seed)


# --------------------------------------------------------------------------------------------------------------- PARITY
@pytest.mark.parametrize("want_index", [False, True], ids=["noindex", "index"])
@pytest.mark.parametrize("dtype", ["f32", "u8", "u16"])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_parity_merged(ctxs, shape, dtype, want_index):
    n, h, w, border = SHAPES[shape]
    qs = rig_qs(n)
    rng = np.random.default_rng(5)
    masks = [rng.random((h - 2 * border) * (w - 2 * border)) >= 0.1 for _ in range(n)]   # a few d = 0: inf coordinates
    data = op.frames_for(masks, h, w, border, dtype, "zero", 17)
    with d2pc.RigSession(ctxs[0], n, w, h, DTC[dtype], [q for q, _ in qs]) as rig:
        for form in (d2pc.FORM_DEFAULT, d2pc.FORM_CV4):
            configure(ctxs, border, d2pc.MODE_PARITY, form)
            got = run_rig(rig, data.frames, data.scale, want_index, pad=dtype == "f32")
            roi_n = (h - 2 * border) * (w - 2 * border)
            assert np.array_equal(got.counts[:n], np.full(n, roi_n)) and got.cap == n * roi_n
            total = check_cloud(got, ctxs, data.frames, qs, data.scale, border, False, form, -np.inf, want_index,
                                f"PARITY {shape} {dtype} form {form}")
            assert total == n * roi_n
        for f, (q, _) in enumerate(qs):
            assert np.array_equal(rig.get_q(f).view(np.uint64), np.asarray(q).view(np.uint64))


def test_parity_without_counts_and_offsets(ctxs):
    n, h, w, border = SHAPES["three"]
    qs = rig_qs(n)
    data = random_frames(n, h, w, "f32", 3)
    configure(ctxs, border, d2pc.MODE_PARITY)
    with d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_F32, [q for q, _ in qs]) as rig:
        want = run_rig(rig, data.frames, 1.0, False)
        cap = want.cap
        keep = to_device(data.frames, False)
        pts = torch.full(((cap + GUARD) * 4,), PT_SENTINEL, dtype=torch.int32, device=DEV)
        rig.process_device(keep[1], 1.0, keep[2], keep[3], pts.data_ptr(), None, cap, None, None, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert np.array_equal(pts.cpu().numpy().view(np.uint32).reshape(-1, 4), want.points)


# -------------------------------------------------------------------------------------------------------------- COMPACT
def mask_sets(n, roi_n):
    rng = np.random.default_rng(29)
    seeded = [rng.random(roi_n) >= 0.3 for _ in range(n)]
    ones, zeros = np.ones(roi_n, dtype=bool), np.zeros(roi_n, dtype=bool)
    last, first = [zeros.copy() for _ in range(n)], [zeros.copy() for _ in range(n)]
    last[n - 1][roi_n - 1] = True
    first[0][0] = True
    rc = list(op.run_counts(roi_n, COMPACT_TILE, 11).values()) + list(op.run_counts(roi_n, COMPACT_TILE, 12).values())
    return {"all": [ones] * n, "middle_empty": [zeros if f == n // 2 else seeded[f] for f in range(n)], "none": [zeros] * n,
            "last_only": last, "first_only": first, "run_counts": rc[:n], "seeded": seeded}


COMPACT_CASES = [(m, "f32", "zero") for m in ("all", "middle_empty", "none", "last_only", "first_only", "run_counts")] + \
    [("seeded", "f32", "floor"), ("seeded", "f32", "nan"), ("seeded", "f32", "inf"), ("run_counts", "u8", "zero"),
     ("seeded", "u8", "floor"), ("run_counts", "u16", "zero"), ("seeded", "u16", "floor")]


@pytest.mark.parametrize("maskset,dtype,kind", COMPACT_CASES, ids=["-".join(c) for c in COMPACT_CASES])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_compact_merged(ctxs, shape, maskset, dtype, kind):
    n, h, w, border = SHAPES[shape]
    roi_n = (h - 2 * border) * (w - 2 * border)
    qs = rig_qs(n)
    valid = mask_sets(n, roi_n)[maskset]
    data = op.frames_for(valid, h, w, border, dtype, "nan" if kind == "inf" else kind, 41)
    if kind == "inf":   # every other hole +inf or -inf instead of NaN
        for fr in data.frames:
            roi = fr[border:h - border, border:w - border]
            holes = np.flatnonzero(np.isnan(roi.reshape(-1)))
            vals = roi.reshape(-1).copy()
            vals[holes[0::3]], vals[holes[1::3]] = np.inf, -np.inf
            roi[:] = vals.reshape(roi.shape)
    with d2pc.RigSession(ctxs[0], n, w, h, DTC[dtype], [q for q, _ in qs]) as rig:
        for form in (d2pc.FORM_DEFAULT, d2pc.FORM_CV4):
            configure(ctxs, border, d2pc.MODE_COMPACT, form, data.dmin)
            got = run_rig(rig, data.frames, data.scale, True, pad=dtype == "f32")
            what = f"COMPACT {shape} {maskset} {dtype} {kind} form {form}"
            assert np.array_equal(got.counts[:n], [int(v.sum()) for v in valid]), what
            total = check_cloud(got, ctxs, data.frames, qs, data.scale, border, True, form, data.dmin, True, what, valid=valid)
            assert total == sum(int(v.sum()) for v in valid)
            if maskset == "middle_empty":
                assert got.counts[n // 2] == 0 and got.offsets[n // 2] == got.offsets[n // 2 + 1]
            if maskset == "none":
                assert total == 0 and np.all(got.points == PT_SENTINEL) and np.all(got.index == IX_SENTINEL)


def test_scan_seam_on_the_device(ctxs):
    """More tiles than two full trips of the scan kernel's loop plus a ragged remainder; compared on the device."""
    n, h, w, border = 9, 800, 1204, 2
    roi_n = (h - 2 * border) * (w - 2 * border)
    tiles = n * -(-roi_n // COMPACT_TILE)
    assert tiles > 2 * SCAN_TRIP and tiles % SCAN_TRIP != 0 and roi_n % COMPACT_TILE != 0, tiles
    qs = rig_qs(n)
    rng = np.random.default_rng(8)
    disp = (rng.integers(72, 960, size=(n, h, w)) / 8.0).astype(np.float32)
    valid = rng.random((n, h, w)) >= 0.3
    disp[~valid] = 0.0
    want_counts = valid[:, border:h - border, border:w - border].reshape(n, -1).sum(axis=1)
    configure(ctxs, border, d2pc.MODE_COMPACT)
    d = torch.from_numpy(disp).to(DEV)
    cap = n * roi_n
    pts = torch.full((cap + GUARD, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((cap + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    with d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_F32, [q for q, _ in qs]) as rig:
        rig.process_device(d.data_ptr(), 1.0, w * 4, h * w * 4, pts.data_ptr(), idx.data_ptr(), cap, counts.data_ptr(),
                           offsets.data_ptr(), s)
        torch.cuda.synchronize()
    got_counts, got_offsets = counts.cpu().numpy(), offsets.cpu().numpy().astype(np.int64)
    assert np.array_equal(got_counts, want_counts)
    assert np.array_equal(got_offsets, np.concatenate([[0], np.cumsum(want_counts)]))
    rpts = torch.empty((roi_n, 4), dtype=torch.int32, device=DEV)
    ridx = torch.empty((roi_n,), dtype=torch.int32, device=DEV)
    rcnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    ok = torch.ones((), dtype=torch.bool, device=DEV)
    for f in range(n):
        ctxs[1].set_q(qs[f][0])
        ctxs[1].process_device(d[f].data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, 1, rpts.data_ptr(), ridx.data_ptr(),
                               roi_n, rcnt.data_ptr(), s)
        a, c = int(got_offsets[f]), int(got_counts[f])
        ok &= (rcnt[0] == c) & torch.equal(pts[a:a + c], rpts[:c]) & torch.equal(idx[a:a + c] - f * w * h, ridx[:c])
    total = int(got_offsets[n])
    ok &= (pts[total:] == PT_SENTINEL).all() & (idx[total:] == IX_SENTINEL).all()
    assert bool(ok)


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT], ids=["parity", "compact"])
def test_one_camera_is_process_device(ctxs, mode):
    h, w, border = 37, 70, 3
    valid = [np.random.default_rng(2).random((h - 2 * border) * (w - 2 * border)) >= 0.3]
    data = op.frames_for(valid, h, w, border, "f32", "zero", 6)
    qs = rig_qs(1)
    configure(ctxs, border, mode)
    with d2pc.RigSession(ctxs[0], 1, w, h, d2pc.DTYPE_F32, [qs[0][0]]) as rig:
        got = run_rig(rig, data.frames, 1.0, True)
    ctxs[1].set_q(qs[0][0])
    rp, ri, rc, roi_n = run_batch(ctxs[1], data.frames, want_index=True)
    c = int(rc[0])
    assert got.counts[0] == c == (roi_n if mode == d2pc.MODE_PARITY else int(valid[0].sum())) and list(got.offsets[:2]) == [0, c]
    assert np.array_equal(got.points[:c], rp[0, :c].view(np.uint32)) and np.array_equal(got.index[:c], ri[0, :c])
    assert np.all(got.points[c:] == PT_SENTINEL) and np.all(got.index[c:] == IX_SENTINEL)


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT], ids=["parity", "compact"])
def test_rig_batch_of_the_torch_plumbing(ctxs, mode):
    """torch_api.RigBatch (buffers + launch + results) gives what the raw call gives."""
    from disparity_to_point_cloud_amd.torch_api import RigBatch
    n, h, w, border = SHAPES["three"]
    qs = rig_qs(n)
    valid = mask_sets(n, (h - 2 * border) * (w - 2 * border))["seeded"]
    data = op.frames_for(valid, h, w, border, "u8", "zero", 13)
    configure(ctxs, border, mode)
    b = RigBatch(ctxs[0], [q for q, _ in qs], h, w, dtype=torch.uint8, want_index=True)
    b.frames.copy_(torch.from_numpy(np.stack(data.frames)))
    b.launch(scale=data.scale)
    pts, idx, counts, offsets = b.results()
    want = run_rig(b.rig, data.frames, data.scale, True)
    total = int(want.offsets[n])
    assert np.array_equal(counts, want.counts[:n]) and np.array_equal(offsets, want.offsets[:n + 1])
    assert np.array_equal(pts.view(np.uint32), want.points[:total]) and np.array_equal(idx, want.index[:total])
    b.rig.close()


# ---------------------------------------------------------------------------------------------------------------- graph
def test_graph_capture_without_warm_up_and_set_q_between_replays(ctxs):
    n, h, w, border = SHAPES["three"]
    roi_n = (h - 2 * border) * (w - 2 * border)
    qs = rig_qs(n)
    valid = mask_sets(n, roi_n)["seeded"]
    data = op.frames_for(valid, h, w, border, "f32", "zero", 77)
    configure(ctxs, border, d2pc.MODE_COMPACT)
    cap = n * roi_n
    keep = to_device(data.frames, False)
    pts = torch.full((cap, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((cap,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=DEV)

    def wipe():
        pts.fill_(PT_SENTINEL), idx.fill_(IX_SENTINEL), counts.fill_(-1), offsets.fill_(-1)
        torch.cuda.synchronize()

    def snapshot():
        torch.cuda.synchronize()
        return [t.cpu().numpy().copy() for t in (pts, idx, counts, offsets)]

    with d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_F32, [q for q, _ in qs]) as rig, \
            d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_F32, [q for q, _ in qs]) as eager_rig:
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):   # the first call this rig ever sees: create allocated everything
            rig.process_device(keep[1], 1.0, keep[2], keep[3], pts.data_ptr(), idx.data_ptr(), cap, counts.data_ptr(),
                               offsets.data_ptr(), torch.cuda.current_stream().cuda_stream)

        def eager():
            wipe()
            eager_rig.process_device(keep[1], 1.0, keep[2], keep[3], pts.data_ptr(), idx.data_ptr(), cap, counts.data_ptr(),
                                     offsets.data_ptr(), torch.cuda.current_stream().cuda_stream)
            return snapshot()

        want = eager()
        assert want[3][n] == sum(int(v.sum()) for v in valid)
        for _ in range(3):
            wipe()
            g.replay()
            assert all(np.array_equal(a, b) for a, b in zip(snapshot(), want))
        new_q = pose_q(qs[1][0])
        rig.set_q(1, new_q)
        eager_rig.set_q(1, new_q)
        wipe()
        g.replay()   # the graph reads the table when it replays
        got = snapshot()
        want2 = eager()
        assert all(np.array_equal(a, b) for a, b in zip(got, want2))
        a, c = int(want[3][1]), int(want[2][1])
        assert not np.array_equal(want2[0][a:a + c], want[0][a:a + c]) and np.array_equal(want2[0][:a], want[0][:a])
        ctxs[1].set_q(new_q)   # ... and equals what a context computes for that Q
        rp, _, rc, _ = run_batch(ctxs[1], [data.frames[1]], want_index=False)
        assert int(rc[0]) == c and np.array_equal(got[0][a:a + c].view(np.uint32), rp[0, :c].view(np.uint32))
        ctxs[0].check_async_error()


# ------------------------------------------------------------------------------------------------------- beyond 4 GiB
@pytest.fixture(scope="module")
def arena():
    t = torch.empty((1 << 32) + (96 << 20), dtype=torch.uint8, device=DEV)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT], ids=["parity", "compact"])
def test_outputs_beyond_4_gib_of_an_allocation(ctxs, arena, mode):
    """Points, indices, counts and offsets all lie past offset 2^32 of one allocation (points 16-byte aligned only);
    equal to the same call into small buffers, and no other byte of the arena changes."""
    n, h, w, border = SHAPES["three"]
    roi_n = (h - 2 * border) * (w - 2 * border)
    qs = rig_qs(n)
    valid = mask_sets(n, roi_n)["seeded"]
    data = op.frames_for(valid, h, w, border, "f32", "zero", 19)
    configure(ctxs, border, mode)
    cap = n * roi_n
    G = 1 << 32
    p_off, i_off, c_off, o_off = G + 4096 + 16, G + (32 << 20) + 4, G + (48 << 20), G + (64 << 20)
    arena.fill_(0xA5)
    keep = to_device(data.frames, True)
    with d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_F32, [q for q, _ in qs]) as rig:
        want = run_rig(rig, data.frames, 1.0, True, pad=True)
        check_cloud(want, ctxs, data.frames, qs, 1.0, border, mode == d2pc.MODE_COMPACT, d2pc.FORM_DEFAULT, -np.inf, True,
                    "small buffers", valid=valid if mode == d2pc.MODE_COMPACT else None)
        base = arena.data_ptr()
        rig.process_device(keep[1], 1.0, keep[2], keep[3], base + p_off, base + i_off, cap, base + c_off, base + o_off,
                           torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    total = int(want.offsets[n])
    regions = {"points": (p_off, total * 16, want.points[:total]), "index": (i_off, total * 4, want.index[:total]),
               "counts": (c_off, n * 4, want.counts[:n]), "offsets": (o_off, (n + 1) * 4, want.offsets[:n + 1])}
    for name, (off, nbytes, expect) in regions.items():
        got = arena[off:off + nbytes].cpu().numpy().view(np.uint32)
        assert np.array_equal(got, expect.reshape(-1)), name
        arena[off:off + nbytes] = 0xA5
    s64 = int(np.array([0xA5] * 8, dtype=np.uint8).view(np.int64)[0])
    dirty = torch.zeros((), dtype=torch.bool, device=DEV)
    for o in range(0, arena.numel(), 1 << 30):
        dirty |= (arena[o:o + (1 << 30)].view(torch.int64) != s64).any()
    assert not bool(dirty), "bytes outside the outputs were written"


@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT], ids=["parity", "compact"])
def test_cloud_larger_than_4_gib(ctxs, mode):
    """17 cameras of 4096 x 4096, every pixel a point: camera 16 starts at point 2^28, byte 2^32 of the cloud, so a point
    address formed in 32 bits would land on camera 0.  The first camera, the last two and the guard behind the cloud are
    compared on the device with d2pc_process_device's output for that camera."""
    n, h, w, border = 17, 4096, 4096, 0
    roi_n = h * w
    assert (n - 1) * roi_n * 16 >= 1 << 32 and n * roi_n < 1 << 32
    qs = rig_qs(n)
    configure(ctxs, border, mode)
    gen = torch.Generator(device=DEV).manual_seed(4)
    d = torch.randint(8, 256, (n, h, w), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)
    cap = n * roi_n
    pts = torch.empty((cap + GUARD, 4), dtype=torch.int32, device=DEV)
    pts[cap:] = PT_SENTINEL
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    with d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_U8, [q for q, _ in qs]) as rig:
        rig.process_device(d.data_ptr(), 0.125, w, h * w, pts.data_ptr(), None, cap, counts.data_ptr(), offsets.data_ptr(), s)
        torch.cuda.synchronize()
        ctxs[0].check_async_error()
    assert np.array_equal(counts.cpu().numpy(), np.full(n, roi_n))
    assert np.array_equal(offsets.cpu().numpy().view(np.uint32), np.arange(n + 1, dtype=np.uint64) * roi_n)
    rpts = torch.empty((roi_n, 4), dtype=torch.int32, device=DEV)
    rcnt = torch.zeros(1, dtype=torch.int32, device=DEV)
    for f in (0, n - 2, n - 1):
        ctxs[1].set_q(qs[f][0])
        ctxs[1].process_device(d[f].data_ptr(), d2pc.DTYPE_U8, 0.125, w, h, w, h * w, 1, rpts.data_ptr(), None, roi_n, rcnt.data_ptr(), s)
        assert torch.equal(pts[f * roi_n:(f + 1) * roi_n], rpts) and int(rcnt[0]) == roi_n, f
    assert bool((pts[cap:] == PT_SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_outputs_untouched(ctxs):
    n, h, w, border = SHAPES["three"]
    roi_n = (h - 2 * border) * (w - 2 * border)
    qs = rig_qs(n)
    data = random_frames(n, h, w, "f32", 9)
    cap = n * roi_n
    keep = to_device(data.frames, False)
    pts = torch.full(((cap + GUARD) * 4,), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((cap + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.full((n,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    offsets = torch.full((n + 1,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    s = torch.cuda.current_stream().cuda_stream

    def call(rig, frames=keep[1], points=None, capacity=cap, c=True, o=True):
        with pytest.raises(d2pc.D2pcError) as e:
            rig.process_device(frames, 1.0, keep[2], keep[3], pts.data_ptr() if points is None else points, idx.data_ptr(), capacity,
                               counts.data_ptr() if c else None, offsets.data_ptr() if o else None, s)
        return e.value.status

    with d2pc.RigSession(ctxs[0], n, w, h, d2pc.DTYPE_F32, [q for q, _ in qs]) as rig:
        configure(ctxs, border, d2pc.MODE_COMPACT)
        assert call(rig, c=False) == INVALID_ARG and call(rig, o=False) == INVALID_ARG
        assert call(rig, capacity=cap - 1) == CAPACITY
        assert call(rig, points=pts.data_ptr() + 8) == INVALID_ARG                 # misaligned d_out_points
        assert call(rig, points=keep[1] + 64) == INVALID_ARG                       # the cloud would overwrite the frames
        assert call(rig, frames=pts.data_ptr() + 16 * 8) == INVALID_ARG            # the frames lie inside the cloud
        ctxs[0].set_reproject_form(d2pc.FORM_CV24)
        assert call(rig) == INVALID_ARG
        ctxs[0].set_mode(d2pc.MODE_PARITY)
        assert call(rig) == INVALID_ARG and call(rig, capacity=0) == INVALID_ARG   # (CV24 still)
        ctxs[0].set_reproject_form(d2pc.FORM_DEFAULT)
        assert call(rig, capacity=cap - 1) == CAPACITY
        for cam in (-1, n, 64):
            with pytest.raises(d2pc.D2pcError) as e:
                rig.set_q(cam, qs[0][0])
            assert e.value.status == INVALID_ARG
            with pytest.raises(d2pc.D2pcError):
                rig.get_q(cam)
        torch.cuda.synchronize()
        for t, sentinel in ((pts, PT_SENTINEL), (idx, IX_SENTINEL), (counts, IX_SENTINEL), (offsets, IX_SENTINEL)):
            assert bool((t == sentinel).all())
        assert bool((keep[0][:n * keep[3]].view(n, h, w * 4) == torch.from_numpy(np.stack(data.frames).view(np.uint8).reshape(n, h, w * 4)).to(DEV)).all())
        # a border wider than the frame: no points, zero counts and offsets, nothing else written
        ctxs[0].set_border(20)
        rig.process_device(keep[1], 1.0, keep[2], keep[3], pts.data_ptr(), idx.data_ptr(), 0, counts.data_ptr(), offsets.data_ptr(), s)
        torch.cuda.synchronize()
        assert bool((counts == 0).all()) and bool((offsets == 0).all()) and bool((pts == PT_SENTINEL).all())
    for bad in (dict(n_cameras=0), dict(n_cameras=65), dict(dtype=d2pc.DTYPE_MONO16), dict(width=0)):
        kw = dict(dict(n_cameras=2, width=w, height=h, dtype=d2pc.DTYPE_F32), **bad)
        with pytest.raises(d2pc.D2pcError):
            capi.RigSession(ctxs[0], kw["n_cameras"], kw["width"], kw["height"], kw["dtype"], np.zeros(16 * kw["n_cameras"]))
