"""d2pc_texture_device on the GPU: PointXYZI / PointXYZRGB records attached behind every producer.  The expected bytes
come from tests/textured_expect.py: the producer's own 16 bytes, the texture word gathered in numpy at the point's
source pixel, three zero words.  Every comparison is of uint32 bit patterns.  tests/README_textured.md has the map."""
import ctypes
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest

import disparity_to_point_cloud_amd as d2pc
import textured_expect as te
from disparity_to_point_cloud_amd import capi
from helpers import assert_points_close

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

DEV = "cuda"
PT_SENTINEL, IX_SENTINEL, OUT_SENTINEL = 0x7FC5A5A5, 0x5A5AA5A5, 0x7FC3C3C3   # patterns no kernel here produces
GUARD = 64                                    # sentinel records kept past every buffer
INVALID_ARG, BAD_DTYPE, BAD_SIZE = 1, 2, 3
FMTS = ["u8", "u16", "f32", "rgb8", "bgr8", "mono8"]
# (rows, cols, border): ROI 16 x 8 = 128 points, less than a block's tile; ROI 64 x 31 = 1,984 points, ragged tiles, several
# blocks; border 0, so that u = 0, u = W - 1 and v = H - 1 are read; two odd widths for the packed 3-byte formats
SHAPES = {"20x12b2": (12, 20, 2), "70x37b3": (37, 70, 3), "20x12b0": (12, 20, 0), "21x13b0": (13, 21, 0), "71x37b3": (37, 71, 3)}
N_FRAMES = 3
SPECIAL_F32 = np.array([0x7FC0BEEF, 0xFFC00001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x7F7FFFFF], dtype=np.uint32)


@pytest.fixture(scope="module")
def ctx():
    with d2pc.Context(q=d2pc.make_q(), border=3, compact_algo=1) as c:
        yield c


def stream():
    return torch.cuda.current_stream().cuda_stream


def dev_i32(a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32).copy()).to(DEV)


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def make_texture(fmt, f, h, w, seed, alloc_frames=None, fill_tail=None):
    """`f` planes of h x w in a device buffer -> SimpleNamespace(planes (numpy, logical), buf, ptr, pitch, fstride).
    u8 / u16 / f32 / mono8: rows 8 bytes longer than they need to be, frames 2 rows further apart.  rgb8 / bgr8: packed,
    pitch 3 W (odd for odd W), the base 1 byte off any alignment.  alloc_frames > f: further planes behind the declared
    ones, every byte fill_tail."""
    rng = np.random.default_rng(seed)
    bpp = te.BYTES_PER_PIXEL[fmt]
    if fmt == "u16":
        planes = rng.integers(0, 65536, size=(f, h, w)).astype(np.uint16)
        planes[0, 0, :2] = (0, 65535)
    elif fmt == "f32":
        bits = rng.integers(0, 1 << 32, size=(f, h, w), dtype=np.uint64).astype(np.uint32)
        bits.reshape(-1)[:len(SPECIAL_F32)] = SPECIAL_F32
        planes = bits.view(np.float32)
    elif bpp == 3:
        planes = rng.integers(0, 256, size=(f, h, w, 3)).astype(np.uint8)
    else:
        planes = rng.integers(0, 256, size=(f, h, w)).astype(np.uint8)
        planes[0, 0, :2] = (0, 255)
    packed = bpp == 3
    pitch = w * bpp + (0 if packed else 8)
    fstride = (h + (0 if packed else 2)) * pitch
    base = 1 if packed else 0
    total = alloc_frames or f
    buf = torch.full((base + total * fstride + 16,), 0x3C, dtype=torch.uint8, device=DEV)
    view = buf.as_strided((f, h, w * bpp), (fstride, pitch, 1), base)
    view.copy_(torch.from_numpy(np.ascontiguousarray(planes).view(np.uint8).reshape(f, h, w * bpp)).to(DEV))
    if total > f:
        buf[base + f * fstride:] = fill_tail
    return SimpleNamespace(planes=planes, buf=buf, ptr=buf.data_ptr() + base, pitch=pitch, fstride=fstride, fmt=fmt)


def attach(ctx, tex, w, h, n_frames, points, index, counts, cloud_points, pstride, ostride, merged=False, border=0,
           out=None):
    """One d2pc_texture_device call into a sentinel-filled buffer -> (n_clouds, ostride, 8) uint32 and the GUARD records
    behind the last cloud."""
    n_clouds = 1 if merged else n_frames
    if out is None:
        out = torch.full(((n_clouds * ostride + GUARD) * 8,), OUT_SENTINEL, dtype=torch.int32, device=DEV)
    pf, tf = te.FORMATS[tex.fmt]
    desc = d2pc.texture_desc_init(
        point_format=pf, texture_format=tf, width=w, height=h, border=border, n_frames=n_frames, merged=int(merged),
        texture=tex.ptr, tex_pitch=tex.pitch, tex_frame_stride=tex.fstride, points=points.data_ptr(),
        index=index.data_ptr() if index is not None else None, counts=counts.data_ptr() if counts is not None else None,
        cloud_points=cloud_points, points_frame_stride_points=pstride, out=out.data_ptr(), out_frame_stride_points=ostride)
    ctx.texture_device(desc, stream())
    torch.cuda.synchronize()
    got = u32(out).reshape(-1, 8)
    return got[:n_clouds * ostride].reshape(n_clouds, ostride, 8), got[n_clouds * ostride:]


def disparities(f, h, w, seed, holes=0.3):
    """float32 disparities in [1, 64) with `holes` of the pixels 0 (W = 0: an infinite point in PARITY, dropped in
    COMPACT)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0, 64.0, size=(f, h, w)).astype(np.float32)
    d[rng.random(size=d.shape) < holes] = 0.0
    return d


def produce(ctx, disp, border, mode, stride, want_index=True):
    """d2pc_process_device over the batch into sentinel-filled buffers -> device tensors (points, index, counts)."""
    f, h, w = disp.shape
    ctx.set_border(border)
    ctx.set_mode(mode)
    d = torch.from_numpy(disp).to(DEV)
    pts = torch.full((f * stride + GUARD, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((f * stride + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV) if want_index else None
    counts = torch.full((f,), -7, dtype=torch.int32, device=DEV)
    ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, f, pts.data_ptr(),
                       idx.data_ptr() if want_index else None, stride, counts.data_ptr(), stream())
    torch.cuda.synchronize()
    ctx.check_async_error()
    return pts, idx, counts


# --------------------------------------------------------------------------------------------------------------- graph
def test_producer_and_attach_captured_without_a_warm_up(ctx):
    """FIRST in this file on purpose: no other file launches k_texture, so in suite order (and when this file runs alone)
    the capture below holds the first launch of the kernel this process makes.  (The code object it lives in may have
    been loaded by the rig's tests.)"""
    h, w, border = 37, 70, 3
    roi_n = (h - 2 * border) * (w - 2 * border)
    stride = roi_n + 5
    disp = disparities(N_FRAMES, h, w, seed=61)
    tex = make_texture("bgr8", N_FRAMES, h, w, seed=62)
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_COMPACT)
    d = torch.from_numpy(disp).to(DEV)
    pts = torch.empty((N_FRAMES * stride, 4), dtype=torch.int32, device=DEV)
    idx = torch.empty((N_FRAMES * stride,), dtype=torch.int32, device=DEV)
    counts = torch.empty((N_FRAMES,), dtype=torch.int32, device=DEV)
    out = torch.empty((N_FRAMES * stride, 8), dtype=torch.int32, device=DEV)
    desc = d2pc.texture_desc_init(
        point_format=d2pc.POINT_XYZRGB, texture_format=d2pc.TEX_BGR8, width=w, height=h, n_frames=N_FRAMES, texture=tex.ptr,
        tex_pitch=tex.pitch, tex_frame_stride=tex.fstride, points=pts.data_ptr(), index=idx.data_ptr(), counts=counts.data_ptr(),
        cloud_points=roi_n, points_frame_stride_points=stride, out=out.data_ptr(), out_frame_stride_points=stride)

    def wipe():
        pts.fill_(PT_SENTINEL), idx.fill_(IX_SENTINEL), counts.fill_(-1), out.fill_(OUT_SENTINEL)
        torch.cuda.synchronize()

    def both():
        s = stream()
        ctx.process_device(d.data_ptr(), d2pc.DTYPE_F32, 1.0, w, h, w * 4, h * w * 4, N_FRAMES, pts.data_ptr(), idx.data_ptr(),
                           stride, counts.data_ptr(), s)
        ctx.texture_device(desc, s)

    ctx.reserve(w, h, N_FRAMES)     # the producer's compaction state (d2pc.h); the attach needs nothing
    wipe()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):       # the first texture call of this shape the library sees
        both()
    torch.cuda.synchronize()
    assert bool((out == OUT_SENTINEL).all()), "capturing must not run anything"
    wipe()
    both()
    torch.cuda.synchronize()
    want = [t.cpu().numpy().copy() for t in (pts, idx, counts, out)]
    cn = want[2].view(np.uint32)
    assert np.all(cn > 0) and np.all(cn < roi_n)
    for f in range(N_FRAMES):
        a, n = f * stride, int(cn[f])
        rec = te.expect_records(want[0].view(np.uint32)[a:a + n], want[1].view(np.uint32)[a:a + n], tex.planes, "bgr8", frame=f)
        assert np.array_equal(want[3].view(np.uint32)[a:a + n], rec)
        assert np.all(want[3].view(np.uint32)[a + n:a + stride] == OUT_SENTINEL)
    for _ in range(2):
        wipe()
        g.replay()
        torch.cuda.synchronize()
        assert all(np.array_equal(t.cpu().numpy(), x) for t, x in zip((pts, idx, counts, out), want))
    ctx.check_async_error()
    del g
    ctx.release_graph_buffers()


# ------------------------------------------------------------------------------------------------- frame-local layout
@pytest.mark.parametrize("fmt", FMTS)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frame_local_parity_and_compact(ctx, shape, fmt):
    h, w, border = SHAPES[shape]
    roi_n = (h - 2 * border) * (w - 2 * border)
    tex = make_texture(fmt, N_FRAMES, h, w, seed=h * w + len(fmt))
    disp = disparities(N_FRAMES, h, w, seed=border + w)
    pstride, ostride = roi_n + 5, roi_n + 7      # clouds off every alignment but the records' own
    # PARITY: with the producer's index and without any -- the same bytes
    pts, idx, counts = produce(ctx, disp, border, d2pc.MODE_PARITY, pstride)
    assert np.all(u32(counts) == roi_n)
    pn, ixn = u32(pts)[:N_FRAMES * pstride].reshape(N_FRAMES, pstride, 4), u32(idx)[:N_FRAMES * pstride].reshape(N_FRAMES, pstride)
    assert not np.isfinite(pn[:, :roi_n].view(np.float32)).all(), "the holes must give non-finite points"
    with_index, tail1 = attach(ctx, tex, w, h, N_FRAMES, pts, idx, counts, roi_n, pstride, ostride)
    no_index, tail2 = attach(ctx, tex, w, h, N_FRAMES, pts, None, None, roi_n, pstride, ostride, border=border)
    assert np.array_equal(with_index, no_index)
    for f in range(N_FRAMES):
        assert np.array_equal(ixn[f, :roi_n], te.roi_pixels(h, w, border))
        want = te.expect_records(pn[f, :roi_n], ixn[f, :roi_n], tex.planes, fmt, frame=f)
        assert np.array_equal(with_index[f, :roi_n], want), (shape, fmt, f)
        assert np.all(with_index[f, roi_n:] == OUT_SENTINEL), "a record past the cloud was written"
    assert np.all(tail1 == OUT_SENTINEL) and np.all(tail2 == OUT_SENTINEL)
    # COMPACT: the survivors and their indices
    pts, idx, counts = produce(ctx, disp, border, d2pc.MODE_COMPACT, pstride)
    cn = u32(counts).astype(np.int64)
    assert np.array_equal(cn, [(disp[f, border:h - border, border:w - border] != 0).sum() for f in range(N_FRAMES)])
    pn, ixn = u32(pts)[:N_FRAMES * pstride].reshape(N_FRAMES, pstride, 4), u32(idx)[:N_FRAMES * pstride].reshape(N_FRAMES, pstride)
    got, tail = attach(ctx, tex, w, h, N_FRAMES, pts, idx, counts, roi_n, pstride, ostride)
    for f in range(N_FRAMES):
        n = int(cn[f])
        assert 0 < n < roi_n
        want = te.expect_records(pn[f, :n], ixn[f, :n], tex.planes, fmt, frame=f)
        assert np.array_equal(got[f, :n], want), (shape, fmt, f)
        assert np.all(got[f, n:] == OUT_SENTINEL), "a record past the count was written"
    assert np.all(tail == OUT_SENTINEL)


# -------------------------------------------------------------------------------- crafted clouds: seams, guard, bit copy
def crafted_cloud(n, n_pixels, seed):
    """n records of arbitrary bits (NaN payloads, +-inf, -0.0 among them: the copy must not look at them) and n pixel
    indices below n_pixels that begin with the corners."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    pts[:len(SPECIAL_F32), 0] = SPECIAL_F32
    pts[:len(SPECIAL_F32), 1] = SPECIAL_F32[::-1]
    pts[1, 3] = 0x7FC00042       # not even the pad is assumed to be 1.0f
    pix = rng.integers(0, n_pixels, size=n).astype(np.uint32)
    pix[:2] = (0, n_pixels - 1)
    return pts, pix


def test_count_seams_failure_mark_and_clamp(ctx):
    """Counts on the seams of a wave of half records (32), of a block (128 pairs) and of a block's tile (512); the in-band failure mark writes nothing; a count above cloud_points is clamped."""
    h, w, cap = 9, 31, 1100
    tex = make_texture("u8", 1, h, w, seed=5)
    pts, pix = crafted_cloud(cap, h * w, seed=6)
    dp, di = dev_i32(pts), dev_i32(pix)
    want = te.expect_records(pts, pix, tex.planes, "u8", frame=0)
    for count in (0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, cap,
                  0xFFFFFFFF, cap + 1, 0xFFFFFFFE):
        counts = dev_i32(np.array([count], dtype=np.uint32))
        got, tail = attach(ctx, tex, w, h, 1, dp, di, counts, cap, cap, cap)
        n = 0 if count == 0xFFFFFFFF else min(count, cap)
        assert np.array_equal(got[0, :n], want[:n]), count
        assert np.all(got[0, n:] == OUT_SENTINEL) and np.all(tail == OUT_SENTINEL), count
    got, _ = attach(ctx, tex, w, h, 1, dp, di, None, cap, cap, cap)      # no counts: cloud_points each
    assert np.array_equal(got[0], want)


@pytest.mark.parametrize("fmt", ["u8", "f32", "bgr8"])
def test_index_beyond_the_declared_planes_reads_nothing(ctx, fmt):
    """Two frames declared inside an allocation of three whose third is all 0xFF: an index into frame 2 (merged) or
    beyond the frame (frame-local) gives word 0 -- it would give 255, NaN or white if it were read."""
    h, w, n = 6, 10, 200
    tex = make_texture(fmt, 2, h, w, seed=8, alloc_frames=3, fill_tail=0xFF)
    pts, pix = crafted_cloud(n, 2 * h * w, seed=9)
    pix[2:8] = (2 * h * w, 2 * h * w + 1, 3 * h * w - 1, 3 * h * w, 0xFFFFFFFF, 1 << 31)
    got, _ = attach(ctx, tex, w, h, 2, dev_i32(pts), dev_i32(pix), None, n, n, n, merged=True)
    want = te.expect_records(pts, pix, tex.planes, fmt)
    assert np.all(want[2:8, 4] == 0) and np.count_nonzero(want[:, 4]) > n // 2
    assert np.array_equal(got[0], want)
    # frame-local: two clouds over the same records; an index at or beyond W * H is outside
    pix2 = np.concatenate([pix, pix]).astype(np.uint32)
    pts2 = np.concatenate([pts, pts])
    got, _ = attach(ctx, tex, w, h, 2, dev_i32(pts2), dev_i32(pix2), None, n, n, n)
    for f in range(2):
        want = te.expect_records(pts, pix, tex.planes, fmt, frame=f)
        assert np.count_nonzero(want[:, 4] == 0) >= n // 3
        assert np.array_equal(got[f], want), f


# ------------------------------------------------------------------------------------------------------- merged layout
def rig_frames(case, n, h, w, border):
    d = disparities(n, h, w, seed=31, holes=0.3)
    if case == "middle_empty":
        d[n // 2] = 0.0
    elif case in ("survivor_first", "survivor_last"):
        d[:] = 0.0
        f, v, u = (0, border, border) if case == "survivor_first" else (n - 1, h - border - 1, w - border - 1)
        d[f, v, u] = 9.5
    return d


@pytest.mark.parametrize("fmt", ["u16", "rgb8"])
@pytest.mark.parametrize("case", ["seeded", "middle_empty", "survivor_first", "survivor_last"])
def test_merged_rig_cloud(ctx, case, fmt):
    n, h, w, border = 5, 12, 20, 2
    roi_n = (h - 2 * border) * (w - 2 * border)
    cap = n * roi_n
    q0 = d2pc.make_q()
    q1 = d2pc.make_q(fx=601.5, fy=598.25, cx=331.75, cy=233.5, baseline=0.12, nx=640, ny=480)
    qs = [q0, q1, q0, q1, q1]
    disp = rig_frames(case, n, h, w, border)
    tex = make_texture(fmt, n, h, w, seed=41)
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_COMPACT)
    d = torch.from_numpy(disp).to(DEV)
    pts = torch.full((cap + GUARD, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((cap + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros(n, dtype=torch.int32, device=DEV)
    offsets = torch.zeros(n + 1, dtype=torch.int32, device=DEV)
    with d2pc.RigSession(ctx, n, w, h, d2pc.DTYPE_F32, qs) as rig:
        rig.process_device(d.data_ptr(), 1.0, w * 4, h * w * 4, pts.data_ptr(), idx.data_ptr(), cap, counts.data_ptr(),
                           offsets.data_ptr(), stream())
        torch.cuda.synchronize()
    total = int(u32(offsets)[n])
    assert total == int((disp[:, border:h - border, border:w - border] != 0).sum())
    # counts = d_offsets + n: the merged cloud's total, read on the device
    got, tail = attach(ctx, tex, w, h, n, pts, idx, offsets[n:], cap, cap, cap, merged=True)
    # the expectation: camera after camera, d2pc_process_device with that camera's Q, textured with that camera's plane
    parts = []
    for f in range(n):
        ctx.set_q(qs[f])
        fp, fi, fc = produce(ctx, disp[f:f + 1], border, d2pc.MODE_COMPACT, roi_n)
        c = int(u32(fc)[0])
        assert c == int(u32(counts)[f])
        parts.append(te.expect_records(u32(fp)[:c], u32(fi)[:c], tex.planes, fmt, frame=f))
    ctx.set_q(q0)
    want = np.concatenate(parts)
    assert len(want) == total and np.array_equal(got[0, :total], want), case
    assert np.array_equal(got[0, :total], te.expect_records(u32(pts)[:total], u32(idx)[:total], tex.planes, fmt))
    assert np.all(got[0, total:] == OUT_SENTINEL) and np.all(tail == OUT_SENTINEL)


# ---------------------------------------------------------------------------------------------------------- addresses
@pytest.fixture(scope="module")
def arena():
    t = torch.empty((1 << 32) + (96 << 20), dtype=torch.uint8, device=DEV)
    yield t
    del t
    torch.cuda.empty_cache()


def test_points_and_out_beyond_4_gib_of_an_allocation(ctx, arena):
    """`points`, `index` and `out` lie past offset 2^32 of one allocation (16-byte aligned only); equal to the same
    call on small buffers, and no other byte of the arena changes."""
    h, w, n = 37, 70, 1984
    tex = make_texture("u16", 1, h, w, seed=51)
    pts, pix = crafted_cloud(n, h * w, seed=52)
    want = te.expect_records(pts, pix, tex.planes, "u16", frame=0)
    G = 1 << 32
    p_off, i_off, o_off = G + 4096 + 16, G + (32 << 20) + 4, G + (64 << 20) + 48
    arena.fill_(0xA5)
    arena[p_off:p_off + n * 16] = dev_i32(pts).view(torch.uint8).reshape(-1)
    arena[i_off:i_off + n * 4] = dev_i32(pix).view(torch.uint8).reshape(-1)
    base = arena.data_ptr()
    desc = d2pc.texture_desc_init(texture_format=d2pc.TEX_U16, width=w, height=h, texture=tex.ptr, tex_pitch=tex.pitch,
                                  points=base + p_off, index=base + i_off, cloud_points=n, out=base + o_off)
    ctx.texture_device(desc, stream())
    torch.cuda.synchronize()
    got = arena[o_off:o_off + n * 32].cpu().numpy().view(np.uint32).reshape(n, 8)
    assert np.array_equal(got, want)
    for off, nbytes in ((p_off, n * 16), (i_off, n * 4), (o_off, n * 32)):
        arena[off:off + nbytes] = 0xA5
    s64 = int(np.array([0xA5] * 8, dtype=np.uint8).view(np.int64)[0])
    dirty = torch.zeros((), dtype=torch.bool, device=DEV)
    for o in range(0, arena.numel(), 1 << 30):
        dirty |= (arena[o:o + (1 << 30)].view(torch.int64) != s64).any()
    assert not bool(dirty), "bytes outside the output were written"


def test_cloud_whose_output_passes_4_gib(ctx):
    """One cloud of 2^27 + 257 records: record 2^27 starts at byte 2^32 of `out`, so a record address formed in 32 bits
    would land on record 0.  Four times as many tiles as one-shot blocks per cloud (2^16), so the blocks' stride loop
    runs.  Compared on the device, slice by slice."""
    n = (1 << 27) + 257
    need = n * (16 + 4 + 32) + (2 << 30)
    if torch.cuda.mem_get_info()[0] < need:
        pytest.skip("the device cannot hold the %.1f GiB of this cloud" % (need / 2 ** 30))
    h, w = 480, 752
    gen = torch.Generator(device=DEV).manual_seed(7)
    texture = torch.randint(0, 256, (h, w), generator=gen, device=DEV, dtype=torch.int32).to(torch.uint8)
    pts = torch.randint(-(1 << 31), (1 << 31) - 1, (n, 4), generator=gen, device=DEV, dtype=torch.int32)
    idx = torch.randint(0, h * w, (n,), generator=gen, device=DEV, dtype=torch.int32)
    out = torch.empty((n + GUARD, 8), dtype=torch.int32, device=DEV)
    out[1 << 27:] = OUT_SENTINEL          # what a wrapped address would leave unwritten, and the guard
    desc = d2pc.texture_desc_init(width=w, height=h, texture=texture.data_ptr(), tex_pitch=w, points=pts.data_ptr(),
                                  index=idx.data_ptr(), cloud_points=n, out=out.data_ptr())
    ctx.texture_device(desc, stream())
    torch.cuda.synchronize()
    flat = texture.reshape(-1)
    step = 1 << 24
    for a in range(0, n, step):
        b = min(a + step, n)
        assert torch.equal(out[a:b, :4], pts[a:b]), a
        word = flat[idx[a:b].long()].to(torch.float32).view(torch.int32)
        assert torch.equal(out[a:b, 4], word), a
        assert not bool(out[a:b, 5:].any()), a
    assert bool((out[n:] == OUT_SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_output_untouched(ctx):
    h, w, border, f = 12, 20, 2, 2
    roi_n = (h - 2 * border) * (w - 2 * border)
    tex8, tex16, tex3 = (make_texture(k, f, h, w, seed=71) for k in ("u8", "u16", "rgb8"))
    pts, pix = crafted_cloud(f * roi_n, h * w, seed=72)
    dp, di = dev_i32(pts), dev_i32(pix)
    counts = dev_i32(np.full(f, roi_n, dtype=np.uint32))
    out = torch.full((f * roi_n + GUARD, 8), OUT_SENTINEL, dtype=torch.int32, device=DEV)
    good = dict(width=w, height=h, border=border, n_frames=f, texture=tex8.ptr, tex_pitch=tex8.pitch, tex_frame_stride=tex8.fstride,
                points=dp.data_ptr(), index=di.data_ptr(), counts=counts.data_ptr(), cloud_points=roi_n,
                points_frame_stride_points=roi_n, out=out.data_ptr(), out_frame_stride_points=roi_n)
    t16 = dict(texture_format=d2pc.TEX_U16, texture=tex16.ptr, tex_pitch=tex16.pitch, tex_frame_stride=tex16.fstride)
    lib = d2pc.load_library()

    def status(**kw):
        desc = d2pc.texture_desc_init(**dict(good, **kw))
        return lib.d2pc_texture_device(ctx.handle, ctypes.byref(desc), stream())

    assert status() == 0 and status(**t16) == 0     # the descriptor the refusals below are one step away from
    torch.cuda.synchronize()
    out.fill_(OUT_SENTINEL)
    assert lib.d2pc_texture_device(ctx.handle, None, stream()) == INVALID_ARG
    assert status(struct_size=108) == INVALID_ARG and status(struct_size=0) == INVALID_ARG
    assert status(texture=None) == INVALID_ARG and status(points=None) == INVALID_ARG and status(out=None) == INVALID_ARG
    # formats
    assert status(point_format=0) == BAD_DTYPE and status(point_format=3) == BAD_DTYPE
    assert status(texture_format=0) == BAD_DTYPE and status(texture_format=7) == BAD_DTYPE
    assert status(point_format=d2pc.POINT_XYZRGB) == BAD_DTYPE                 # u8 belongs to XYZI
    assert status(texture_format=d2pc.TEX_MONO8) == BAD_DTYPE                    # mono8 to XYZRGB
    assert status(texture_format=d2pc.TEX_RGB8, texture=tex3.ptr, tex_pitch=tex3.pitch, tex_frame_stride=tex3.fstride) == BAD_DTYPE
    assert status(point_format=d2pc.POINT_XYZRGB, texture_format=d2pc.TEX_F32) == BAD_DTYPE
    # sizes
    for kw in (dict(width=0), dict(height=-1), dict(n_frames=0), dict(border=-1), dict(cloud_points=0),
               dict(cloud_points=1 << 32), dict(n_frames=65536), dict(width=1 << 16, height=1 << 16)):
        assert status(**kw) == BAD_SIZE, kw
    assert status(merged=1, width=1 << 15, height=1 << 15, n_frames=5) == BAD_SIZE     # 5 x 2^30 pixels: no 32-bit index
    # the PARITY layout
    assert status(index=None, merged=1) == INVALID_ARG
    assert status(index=None, cloud_points=roi_n - 1) == BAD_SIZE and status(index=None, border=border + 1) == BAD_SIZE
    assert status(index=None, border=6) == BAD_SIZE                              # an empty ROI
    # alignment
    assert status(points=dp.data_ptr() + 8) == INVALID_ARG and status(out=out.data_ptr() + 4) == INVALID_ARG
    assert status(index=di.data_ptr() + 2) == INVALID_ARG and status(counts=counts.data_ptr() + 1) == INVALID_ARG
    assert status(**dict(t16, texture=tex16.ptr + 1)) == INVALID_ARG
    assert status(**dict(t16, tex_pitch=tex16.pitch + 1)) == INVALID_ARG
    assert status(**dict(t16, tex_frame_stride=tex16.fstride + 1)) == INVALID_ARG
    assert status(texture_format=d2pc.TEX_F32, tex_pitch=w * 4 + 2) == INVALID_ARG
    # the texture plane
    assert status(tex_pitch=w - 1) == BAD_SIZE and status(**dict(t16, tex_pitch=2 * w - 2)) == BAD_SIZE
    assert status(tex_frame_stride=(h - 1) * tex8.pitch + w - 1) == BAD_SIZE
    assert status(tex_pitch=1 << 32) == BAD_SIZE
    # frame strides
    assert status(points_frame_stride_points=roi_n - 1) == BAD_SIZE and status(out_frame_stride_points=roi_n - 1) == BAD_SIZE
    # ... or so large that the hull of the clouds would wrap 64 bits (2^59 x 32 B = 2^64) and hide an overlap
    for big in ((1 << 40) + 1, 1 << 59, (1 << 60) + roi_n):
        assert status(points_frame_stride_points=big) == BAD_SIZE and status(out_frame_stride_points=big) == BAD_SIZE, big
    assert status(out_frame_stride_points=1 << 59, points=out.data_ptr() + 32) == BAD_SIZE    # (was: accepted, overlapping)
    assert status(tex_frame_stride=(1 << 46) + 1) == BAD_SIZE and status(tex_frame_stride=1 << 63) == BAD_SIZE
    # `out` over an input
    assert status(out=dp.data_ptr() + 16 * (f * roi_n - 1)) == INVALID_ARG      # the last point
    assert status(points=out.data_ptr() + 32 * (f * roi_n) - 16) == INVALID_ARG
    assert status(index=out.data_ptr() + 64) == INVALID_ARG and status(counts=out.data_ptr() + 32 * roi_n) == INVALID_ARG
    assert status(texture=out.data_ptr() + 32) == INVALID_ARG
    assert "overlaps" in lib.d2pc_last_error(ctx.handle).decode()
    torch.cuda.synchronize()
    assert bool((out == OUT_SENTINEL).all()), "a refused call wrote the output"
    assert np.array_equal(u32(dp).reshape(-1, 4), pts) and np.array_equal(u32(di), pix)
    # one cloud: the frame strides are not looked at
    assert status(n_frames=1, points_frame_stride_points=0, out_frame_stride_points=0, tex_frame_stride=0) == 0
    assert status(merged=1, cloud_points=f * roi_n, points_frame_stride_points=0, out_frame_stride_points=0) == 0
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ the two nodes joined
def test_fused_depth_map_textured_with_the_combined_score(ctx):
    """FUSED_DEPTH_MAP through the callback body (COMPACT, index), textured with the matching cropped VIEW of
    COMBINED_SCORE: the pointer offset by the node's crop, the node's pitch."""
    from test_colorize_cpu import structured
    cols, rows = 188, 120
    rng = np.random.default_rng(81)
    node = d2pc.FusionNode(ctx, cols, rows, -2, 4)
    cuda = lambda a: torch.from_numpy(a).to(DEV)  # noqa: E731
    node.disparity_1(cuda(rng.integers(0, 256, size=(rows, cols)).astype(np.uint8)))
    node.matching_score_1(cuda((structured(rng, rows, cols) // 3).astype(np.uint8)))
    node.matching_score_2(cuda((structured(rng, rows, cols) // 3).astype(np.uint8)))
    topics = node.disparity_2(cuda(rng.integers(0, 256, size=(rows, cols)).astype(np.uint8)))
    fused, score = topics["fused_depth_map"], topics["combined_score"]
    fh, fw = fused.shape
    left, right, top, bottom = 0, 40, 30, 10           # cropMat of publishFusedDepthMap
    assert tuple(score.shape) == (fh + top + bottom, fw + left + right)
    border = 4
    roi_n = (fh - 2 * border) * (fw - 2 * border)
    ctx.set_border(border)
    ctx.set_mode(d2pc.MODE_COMPACT)
    pts = torch.full((roi_n + GUARD, 4), PT_SENTINEL, dtype=torch.int32, device=DEV)
    idx = torch.full((roi_n + GUARD,), IX_SENTINEL, dtype=torch.int32, device=DEV)
    counts = torch.zeros(1, dtype=torch.int32, device=DEV)
    ctx.process_mono_device(fused.data_ptr(), d2pc.DTYPE_U8, fw, fh, fused.stride(0), 0, 1, 0, 0.125, pts.data_ptr(),
                            idx.data_ptr(), roi_n, counts.data_ptr(), stream())
    out = torch.full((roi_n + GUARD, 8), OUT_SENTINEL, dtype=torch.int32, device=DEV)
    desc = d2pc.texture_desc_init(width=fw, height=fh, texture=score.data_ptr() + top * score.stride(0) + left,
                                  tex_pitch=score.stride(0), points=pts.data_ptr(), index=idx.data_ptr(),
                                  counts=counts.data_ptr(), cloud_points=roi_n, out=out.data_ptr())
    ctx.texture_device(desc, stream())
    torch.cuda.synchronize()
    ctx.check_async_error()
    n = int(u32(counts)[0])
    fz, sc = fused.cpu().numpy(), score.cpu().numpy()
    assert n == int((fz[border:fh - border, border:fw - border] != 0).sum()) and n > roi_n // 8
    got, ix = u32(out)[:n], u32(idx)[:n].astype(np.int64)
    v, u = ix // fw, ix % fw
    assert np.array_equal(got[:, 4].view(np.float32), sc[v + top, u + left].astype(np.float32))
    assert len(np.unique(got[:, 4])) > 2, "a flat score would prove nothing"
    assert np.array_equal(got, te.expect_records(u32(pts)[:n], ix, sc[None, top:top + fh, left:left + fw], "u8", frame=0))
    assert np.all(u32(out)[n:] == OUT_SENTINEL)


# ------------------------------------------------------------------------------------------------------------ plumbing
@pytest.mark.parametrize("mode", [d2pc.MODE_PARITY, d2pc.MODE_COMPACT], ids=["parity", "compact"])
def test_torch_helper_equals_the_raw_call(ctx, mode):
    from disparity_to_point_cloud_amd.torch_api import DeviceBatch, RigBatch, texture_cloud
    h, w, border, f = 37, 71, 3, 3
    roi_n = (h - 2 * border) * (w - 2 * border)
    ctx.set_border(border)
    ctx.set_mode(mode)
    disp = disparities(f, h, w, seed=91)
    b = DeviceBatch(ctx, f, h, w, want_index=True)
    b.disp.copy_(torch.from_numpy(disp))
    b.launch()
    rng = np.random.default_rng(92)
    image = rng.integers(0, 256, size=(f, h + 2, w + 3, 3)).astype(np.uint8)
    view = torch.from_numpy(image).to(DEV)[:, 1:h + 1, 2:w + 2]            # a cropped view: free row and frame strides
    compact = mode == d2pc.MODE_COMPACT
    ctx.set_mode(d2pc.MODE_COMPACT if not compact else d2pc.MODE_PARITY)   # the meta describes the cloud, not the context
    rec, meta = texture_cloud(ctx, b.points, view, index=b.index if compact else None, counts=b.counts, rgb="rgb8",
                              is_dense=compact)
    ctx.set_mode(mode)
    assert tuple(rec.shape) == (f, b.stride, 8) and rec.dtype == torch.float32
    # (without n_points the meta describes a cloud's capacity: the ROI without an index, the buffer's stride with one)
    assert (meta.point_step, meta.width, meta.is_dense, meta.fields[3].name) == (32, b.stride if compact else roi_n, int(compact), b"rgb")
    assert texture_cloud(ctx, b.points, view, index=b.index, counts=b.counts, rgb="rgb8", n_points=7, out=rec)[1].row_step == 224
    tex = SimpleNamespace(fmt="rgb8", ptr=view.data_ptr(), pitch=view.stride(1), fstride=view.stride(0))
    raw, _ = attach(ctx, tex, w, h, f, b.points, b.index, b.counts, roi_n, b.stride, b.stride)
    cn = u32(b.counts)
    pn, ixn = u32(b.points), u32(b.index)
    for k in range(f):
        n = int(cn[k])
        assert n == (roi_n if not compact else int((disp[k, border:h - border, border:w - border] != 0).sum()))
        assert np.array_equal(u32(rec)[k, :n], raw[k, :n])
        assert np.array_equal(raw[k, :n], te.expect_records(pn[k, :n], ixn[k, :n], image[:, 1:h + 1, 2:w + 2], "rgb8", frame=k))
    assert rec.view(torch.uint8).shape[-1] == 32
    # a rig's merged cloud with a float32 plane
    qs = [d2pc.make_q()] * f
    rb = RigBatch(ctx, qs, h, w, want_index=True)
    rb.frames.copy_(torch.from_numpy(disp))
    rb.launch()
    plane = torch.from_numpy(rng.uniform(0, 1, size=(f, h, w)).astype(np.float32)).to(DEV)
    rec, meta = texture_cloud(ctx, rb.points, plane, index=rb.index, counts=rb.offsets[f:], merged=True, is_dense=compact)
    pts, idx, _, offsets = rb.results()
    total = int(offsets[-1])
    assert tuple(rec.shape) == (f * roi_n, 8) and meta.fields[3].name == b"intensity" and meta.is_dense == int(compact)
    assert np.array_equal(u32(rec)[:total], te.expect_records(pts, idx, plane.cpu().numpy(), "f32"))
    rb.rig.close()


def test_xyzi_blob_82x82_on_the_device(golden_dir):
    """The committed PointXYZI blob: xyz within the project's parity bar of the committed points, the rest exact."""
    import sys
    sys.path.insert(0, golden_dir)
    import make_textured_golden as gen
    base = json.load(open(os.path.join(golden_dir, "pointcloud2_82x82.json")))
    gold = json.load(open(os.path.join(golden_dir, "pointcloud2_xyzi_82x82.json")))
    q = np.array([float.fromhex(x) for x in base["q_hex"]])
    disp = np.full((1, 82, 82), 4.0, dtype=np.float32)
    disp[0, 40:42, 40:42] = np.array(base["roi_disparities"], dtype=np.float32).reshape(2, 2)
    with d2pc.Context(q=q) as c:
        pts, _, _ = produce(c, disp, 40, d2pc.MODE_PARITY, 4, want_index=False)
        image = torch.from_numpy(gen.texture_82x82()).to(DEV)
        tex = SimpleNamespace(fmt="u8", ptr=image.data_ptr(), pitch=82, fstride=0)
        got, _ = attach(c, tex, 82, 82, 1, pts, None, None, 4, 4, 4, border=40)
    want = np.frombuffer(bytes.fromhex(gold["data_hex"]), dtype=np.uint32).reshape(4, 8)
    assert np.array_equal(got[0, :, 3:], want[:, 3:])
    assert_points_close(got[0, :, :4].copy().view(np.float32), want[:, :4].copy().view(np.float32), max_ulp=1)
