"""torch plumbing around d2pc_process_device: device memory and streams come
from torch, the work is done by libd2pc.so's HIP kernels.  No torch op ever
computes a point here."""
import numpy as np
import torch

from . import capi

_T2DT = {torch.float32: capi.DTYPE_F32, torch.uint8: capi.DTYPE_U8, torch.uint16: capi.DTYPE_U16}


class DeviceBatch:
    """Pre-allocated device buffers for a batch of equally sized frames."""

    def __init__(self, ctx: capi.Context, n_frames: int, height: int, width: int, dtype=torch.float32,
                 want_index=False, device="cuda:0", reserve=True):
        cfg = ctx.config()
        self.ctx, self.n_frames, self.height, self.width = ctx, n_frames, height, width
        self.roi_n = capi.roi_points(width, height, cfg.border)
        # frame outputs start on 256-byte boundaries (16 points)
        self.stride = max((self.roi_n + 15) // 16 * 16, 16)
        self.device = torch.device(device)
        self.disp = torch.empty((n_frames, height, width), dtype=dtype, device=self.device)
        self.points = torch.empty((n_frames, self.stride, 4), dtype=torch.float32, device=self.device)
        self.index = (torch.empty((n_frames, self.stride), dtype=torch.int32, device=self.device)
                      if want_index else None)
        self.counts = torch.zeros((n_frames,), dtype=torch.int32, device=self.device)
        if reserve:   # (so that a capture finds its compaction state; False: the first eager launch allocates it)
            ctx.reserve(width, height, n_frames)

    def launch(self, scale=1.0, stream=None):
        """Enqueue one pass over the whole batch on `stream` (default: torch's
        current stream).  Asynchronous."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        d = self.disp
        self.ctx.process_device(
            d.data_ptr(), _T2DT[d.dtype], scale, self.width, self.height, d.stride(1) * d.element_size(),
            d.stride(0) * d.element_size(), self.n_frames, self.points.data_ptr(),
            self.index.data_ptr() if self.index is not None else None, self.stride, self.counts.data_ptr(),
            s.cuda_stream)

    def results(self):
        """Synchronise and copy back: list of (points[, index]) per frame."""
        torch.cuda.synchronize(self.device)
        counts = self.counts.cpu().numpy().astype(np.int64)
        pts = self.points.cpu().numpy()
        idx = self.index.cpu().numpy().view(np.uint32) if self.index is not None else None
        out = []
        for f in range(self.n_frames):
            n = int(counts[f])
            out.append((pts[f, :n].copy(), idx[f, :n].copy() if idx is not None else None))
        return out


class RigBatch:
    """Pre-allocated device buffers for a camera rig: n cameras of one size and dtype, one Q each (`qs`: n x 16), ONE
    merged cloud per launch (capi.RigSession).  The buffers are sized for the context's border at construction."""

    def __init__(self, ctx: capi.Context, qs, height: int, width: int, dtype=torch.float32, want_index=False,
                 device="cuda:0"):
        qs = np.asarray(qs, dtype=np.float64).reshape(-1, 16)
        self.ctx, self.n_cameras, self.height, self.width = ctx, len(qs), height, width
        self.rig = capi.RigSession(ctx, self.n_cameras, width, height, _T2DT[dtype], qs)
        self.capacity = int(self.rig.geometry().capacity_points)
        self.device = torch.device(device)
        self.frames = torch.empty((self.n_cameras, height, width), dtype=dtype, device=self.device)
        self.points = torch.empty((max(self.capacity, 1), 4), dtype=torch.float32, device=self.device)
        self.index = torch.empty((max(self.capacity, 1),), dtype=torch.int32, device=self.device) if want_index else None
        self.counts = torch.zeros((self.n_cameras,), dtype=torch.int32, device=self.device)
        self.offsets = torch.zeros((self.n_cameras + 1,), dtype=torch.int32, device=self.device)

    def launch(self, scale=1.0, stream=None):
        """Enqueue one call over the rig's frames on `stream` (default: torch's current stream).  Asynchronous."""
        s = stream if stream is not None else torch.cuda.current_stream(self.device)
        d = self.frames
        self.rig.process_device(d.data_ptr(), scale, d.stride(1) * d.element_size(), d.stride(0) * d.element_size(),
                                self.points.data_ptr(), self.index.data_ptr() if self.index is not None else None,
                                self.capacity, self.counts.data_ptr(), self.offsets.data_ptr(), s.cuda_stream)

    def results(self):
        """Synchronise and copy back: (points, index or None, counts, offsets) of the merged cloud."""
        torch.cuda.synchronize(self.device)
        offsets = self.offsets.cpu().numpy().view(np.uint32).astype(np.int64)
        counts = self.counts.cpu().numpy().view(np.uint32).astype(np.int64)
        n = int(offsets[-1])
        idx = self.index[:n].cpu().numpy().view(np.uint32) if self.index is not None else None
        return self.points[:n].cpu().numpy(), idx, counts, offsets


_T2TEX = {torch.uint8: capi.TEX_U8, torch.uint16: capi.TEX_U16, torch.float32: capi.TEX_F32}


def texture_cloud(ctx: capi.Context, points, texture, index=None, counts=None, merged=False, rgb=None, border=None,
                  n_points=None, is_dense=False, out=None, stream=None):
    """d2pc_texture_device on torch CUDA tensors: the 32-byte PointXYZI / PointXYZRGB records of a cloud this library
    made (DeviceBatch / RigBatch or any d2pc_process*_device result) and a per-pixel plane of the source frames.

    points: (F, stride, 4) float32, one cloud per frame (DeviceBatch.points), or (capacity, 4): one frame's cloud, or
    with merged=True a rig's merged cloud (RigBatch.points).  index / counts: the producer's tensors; for a rig pass
    counts = offsets[n:].  index=None is the PARITY layout (`border` defaults to the context's).
    texture: (F, H, W) or (H, W) of uint8 / uint16 / float32 -> XYZI; with rgb="mono8" a uint8 plane -> XYZRGB;
    (F, H, W, 3) or (H, W, 3) uint8 with rgb="rgb8" / "bgr8" -> XYZRGB.  Unit sample stride; row and frame strides
    are free, so cropped views work.
    Returns (records, meta): records as float32 of shape points.shape[:-1] + (8,) (`.view(torch.uint8)` gives the
    PointCloud2 bytes), written for each cloud's count only; meta = d2pc_textured_cloud_meta for n_points (default:
    the capacity of one cloud, which in PARITY is the cloud) and is_dense -- properties of the CLOUD, which may have
    been made earlier and in another mode than the context is in now: a COMPACT cloud passes is_dense=True and, once
    it has read the count, n_points.  Asynchronous on `stream` (default: torch's current
    stream); no torch op computes anything here."""
    assert points.is_cuda and points.dtype == torch.float32 and points.shape[-1] == 4 and points.is_contiguous()
    assert points.dim() in (2, 3) and not (merged and points.dim() == 3)
    packed = rgb in ("rgb8", "bgr8")
    assert rgb in (None, "mono8", "rgb8", "bgr8") and texture.is_cuda
    planes = texture.dim() - (1 if packed else 0)
    assert planes in (2, 3) and (not packed or (texture.shape[-1] == 3 and texture.stride(-1) == 1))
    col = -2 if packed else -1
    assert texture.stride(col) == (3 if packed else 1)
    f = texture.shape[0] if planes == 3 else 1
    h, w = texture.shape[col - 1], texture.shape[col]
    if rgb is not None:
        assert texture.dtype == torch.uint8
        fmt = {"mono8": capi.TEX_MONO8, "rgb8": capi.TEX_RGB8, "bgr8": capi.TEX_BGR8}[rgb]
    else:
        fmt = _T2TEX[texture.dtype]
    es = texture.element_size()
    n_clouds = 1 if merged else f
    assert (points.shape[0] if points.dim() == 3 else 1) == n_clouds
    cap = points.shape[-2]
    if out is None:
        out = torch.empty(tuple(points.shape[:-1]) + (8,), dtype=torch.float32, device=points.device)
    assert out.is_cuda and out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == tuple(points.shape[:-1]) + (8,)
    cloud_points = cap
    if index is None:
        border = ctx.config().border if border is None else border
        cloud_points = capi.roi_points(w, h, border)
    else:
        assert index.is_cuda and index.element_size() == 4 and index.is_contiguous() and tuple(index.shape) == tuple(points.shape[:-1])
    if counts is not None:
        assert counts.is_cuda and counts.element_size() == 4 and counts.is_contiguous() and counts.numel() >= n_clouds
    desc = capi.texture_desc_init(
        point_format=capi.POINT_XYZI if rgb is None else capi.POINT_XYZRGB, texture_format=fmt, width=w, height=h,
        border=border or 0, n_frames=f, merged=int(bool(merged)), texture=texture.data_ptr(),
        tex_pitch=texture.stride(col - 1) * es, tex_frame_stride=texture.stride(0) * es if planes == 3 else 0,
        points=points.data_ptr(), index=index.data_ptr() if index is not None else None,
        counts=counts.data_ptr() if counts is not None else None, cloud_points=cloud_points,
        points_frame_stride_points=cap, out=out.data_ptr(), out_frame_stride_points=cap)
    s = stream if stream is not None else torch.cuda.current_stream(points.device)
    ctx.texture_device(desc, s.cuda_stream)
    meta = capi.textured_cloud_meta(desc.point_format, cloud_points if n_points is None else n_points, is_dense)
    return out, meta


def fuse_planes(ctx: capi.Context, planes, rule=capi.FUSE_GRAD_FILTER, crop=(0, 40, 30, 10), want_combined=True,
                stream=None):
    """d2pc_fuse_device on torch uint8 CUDA tensors.

    planes = (depth1, depth2, score1, score2, grad1, grad2), each (H, W) or (F, H, W) with unit
    column stride (row/frame strides are free, so cropped views work).  Returns (fused, combined or
    None) as new tensors; asynchronous on `stream` (default: torch's current stream)."""
    assert len(planes) == 6
    ref = planes[0]
    batched = ref.dim() == 3
    shape = tuple(ref.shape)
    f, h, w = (shape if batched else (1,) + shape)
    l, r, t, b = crop
    desc = capi.fuse_desc_init()
    desc.rule, desc.width, desc.height, desc.n_frames = rule, w, h, f
    desc.crop_left, desc.crop_right, desc.crop_top, desc.crop_bottom = l, r, t, b
    for i, p in enumerate(planes):
        if p is None:
            assert i >= 4 and not want_combined
            continue
        assert p.is_cuda and p.dtype == torch.uint8 and tuple(p.shape) == shape and p.stride(-1) == 1
        desc.planes[i] = p.data_ptr()
        desc.pitch[i] = p.stride(-2)
        desc.frame_stride[i] = p.stride(0) if batched else 0
    oh, ow = max(h - t - b, 0), max(w - l - r, 0)
    fused = torch.empty((f, oh, ow), dtype=torch.uint8, device=ref.device)
    combined = torch.empty((f, h, w), dtype=torch.uint8, device=ref.device) if want_combined else None
    desc.fused = fused.data_ptr() if fused.numel() else ref.new_empty(1).data_ptr()
    desc.fused_pitch, desc.fused_frame_stride = max(ow, 1), max(ow, 1) * oh
    if want_combined:
        desc.combined, desc.combined_pitch, desc.combined_frame_stride = combined.data_ptr(), w, w * h
    s = stream if stream is not None else torch.cuda.current_stream(ref.device)
    ctx.fuse_device(desc, s.cuda_stream)
    if not batched:
        fused = fused[0]
        combined = combined[0] if want_combined else None
    return fused, combined


def score_filter(ctx: capi.Context, frames, square, direction, form=capi.SCORE_FORM_CV4, want_grad=False, stream=None):
    """d2pc_score_filter_device on a torch uint8 CUDA tensor: the matching-score pre-filter of MatchingScoreCb1/2.

    frames: (H, W) or (F, H, W) with unit column stride (row/frame strides are free, so views work); camera 2's
    frames already rotated.  square = (x, y, n) from crop_to_square; direction 0 = Sobel(0,2) (camera 1), 1 =
    Sobel(2,0) (camera 2); form = SCORE_FORM_CV4 / SCORE_FORM_CV3.  Returns (out, grad or None) as new (F,) n x n
    tensors; asynchronous on `stream` (default: torch's current stream)."""
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (2, 3) and frames.stride(-1) == 1
    batched = frames.dim() == 3
    f, h, w = tuple(frames.shape) if batched else (1,) + tuple(frames.shape)
    x, y, n = square
    desc = capi.score_filter_desc_init()
    desc.direction, desc.form = direction, form
    desc.width, desc.height, desc.n_frames = w, h, f
    desc.x, desc.y, desc.n = x, y, n
    desc.src, desc.src_pitch = frames.data_ptr(), frames.stride(-2)
    desc.src_frame_stride = frames.stride(0) if batched else 0
    out = torch.empty((f, n, n), dtype=torch.uint8, device=frames.device)
    desc.out, desc.out_pitch, desc.out_frame_stride = out.data_ptr(), n, n * n
    grad = None
    if want_grad:
        grad = torch.empty((f, n, n), dtype=torch.uint8, device=frames.device)
        desc.grad, desc.grad_pitch, desc.grad_frame_stride = grad.data_ptr(), n, n * n
    s = stream if stream is not None else torch.cuda.current_stream(frames.device)
    ctx.score_filter_device(desc, s.cuda_stream)
    if not batched:
        out = out[0]
        grad = grad[0] if want_grad else None
    return out, grad


def colorize(ctx: capi.Context, frames, view=None, rotate_cw=False, want_gray=False, stream=None):
    """d2pc_colorize_device on a torch uint8 CUDA tensor: the view cropToSquare takes in DisparityCb1/2 and its
    colorizeDepth, in one launch.

    frames: (H, W) or (F, H, W) with unit column stride (row/frame strides are free, so views work).  rotate_cw: take
    the view of the frames rotated 90 degrees clockwise (camera 2) without materialising them.  view = (x, y, w, h)
    in the (rotated) frame's coordinates, or (x, y, n) from crop_to_square, or None for the whole plane.  Returns
    (rgb (F,) h x w x 3, gray (F,) h x w or None) as new tensors; asynchronous on `stream` (default: torch's current
    stream)."""
    assert frames.is_cuda and frames.dtype == torch.uint8 and frames.dim() in (2, 3) and frames.stride(-1) == 1
    batched = frames.dim() == 3
    f, rows, cols = tuple(frames.shape) if batched else (1,) + tuple(frames.shape)
    fw, fh = (rows, cols) if rotate_cw else (cols, rows)
    if view is None:
        view = (0, 0, fw, fh)
    elif len(view) == 3:
        view = (view[0], view[1], view[2], view[2])
    x, y, w, h = view
    desc = capi.colorize_desc_init()
    desc.rotate_cw, desc.cols, desc.rows, desc.n_frames = int(bool(rotate_cw)), cols, rows, f
    desc.x, desc.y, desc.w, desc.h = x, y, w, h
    desc.src, desc.src_pitch = frames.data_ptr(), frames.stride(-2)
    desc.src_frame_stride = frames.stride(0) if batched else 0
    shape = (f, max(h, 0), max(w, 0))
    rgb = torch.empty(shape + (3,), dtype=torch.uint8, device=frames.device)
    desc.rgb, desc.rgb_pitch, desc.rgb_frame_stride = rgb.data_ptr(), 3 * w, 3 * w * h
    gray = None
    if want_gray:
        gray = torch.empty(shape, dtype=torch.uint8, device=frames.device)
        desc.gray, desc.gray_pitch, desc.gray_frame_stride = gray.data_ptr(), w, w * h
    s = stream if stream is not None else torch.cuda.current_stream(frames.device)
    ctx.colorize_device(desc, s.cuda_stream)
    if not batched:
        rgb = rgb[0]
        gray = gray[0] if want_gray else None
    return rgb, gray
