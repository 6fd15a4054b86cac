// d2pc_capi_mono.hip -- what happens to a mono image before the reprojection, on the device (reference cpp:50-61):
// cv_bridge's mono16 rescale, cv::medianBlur, and the whole callback body for a resident batch (d2pc_process_mono_device).
// The chain rescale -> median(ROI) is written once, here (prepare_mono, also for d2pc_capi_host.hip and the laboratory's overlap).
#include "d2pc_ctx.hpp"

using namespace d2pc;
using namespace d2pc::host;

namespace d2pc {
namespace host {

int check_median(d2pc_ctx *ctx, bool eight_bit, int ksize) {
  if (eight_bit && median_ksize_supported(ksize)) return D2PC_OK;
  return fail(ctx, D2PC_ERR_INVALID_ARG, "median needs 8-bit (or MONO16) input and a ksize in {3,5,7,9,11} (got %d)", ksize);
}

MedianArgs median_args(const d2pc_ctx *ctx, int width, int height, int n_frames, size_t src_pitch, size_t src_frame,
                       size_t dst_pitch, size_t dst_frame) {
  MedianArgs m;
  m.algo = ctx->median_algo;
  m.width = uint32_t(width);
  m.height = uint32_t(height);
  m.n_frames = uint32_t(n_frames);
  m.src_row_stride = uint32_t(src_pitch);
  m.dst_row_stride = uint32_t(dst_pitch);
  m.src_frame_stride = src_frame;
  m.dst_frame_stride = dst_frame;
  return m;
}

// cpp:55-57 + cpp:69-72: the reference filters the whole image and then reads only the inset ROI ("Removing
// borders" -- the inset exists to hide the filter's border artefacts).  The fused entry points therefore
// compute the median of the ROI pixels only (25.5 % fewer at the native 752x480, border 40); the windows
// still read the unfiltered image up to its true edges, so every ROI pixel equals the whole-image result.
void median_roi_only(MedianArgs &m, const Geom &g, int height) {
  const uint32_t roi_h = uint32_t(height) > 2u * g.border ? uint32_t(height) - 2u * g.border : 0u;
  if (g.roi_w == 0 || roi_h == 0) return;
  m.out_x0 = m.out_y0 = g.border;
  m.out_w = g.roi_w;
  m.out_h = roi_h;
}

int prepare_mono(d2pc_ctx *ctx, Frames *in, int width, int height, int n_frames, bool rescale, int ksize, void *d_cvt,
                 void *d_med, size_t kpitch, size_t kframe, const Geom &roi, hipStream_t s) {
  if (rescale) {
    D2PC_HIP(ctx, launch_mono16_to_mono8(in->p, d_cvt, median_args(ctx, width, height, n_frames, in->pitch, in->frame, kpitch, kframe), s));
    *in = Frames{d_cvt, kpitch, kframe};
  }
  if (ksize > 1) {
    MedianArgs m = median_args(ctx, width, height, n_frames, in->pitch, in->frame, kpitch, kframe);
    median_roi_only(m, roi, height);
    D2PC_HIP(ctx, launch_median(in->p, d_med, m, ksize, s));
    *in = Frames{d_med, kpitch, kframe};
  }
  return D2PC_OK;
}

}  // namespace host
}  // namespace d2pc

extern "C" {

int d2pc_mono16_to_mono8_device(d2pc_ctx *ctx, const void *d_src, int width, int height, size_t src_row_stride,
                                size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_row_stride,
                                size_t dst_frame_stride, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d_src || !d_dst) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  if (width <= 0 || height <= 0 || n_frames <= 0 || n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", width, height, n_frames);
  const Plane src{d_src, src_row_stride, src_frame_stride, size_t(width) * 2, height};  // rows of uint16 samples
  const Plane dst{d_dst, dst_row_stride, dst_frame_stride, size_t(width), height};
  if (!src.fits(n_frames, Bound32::Pitch) || !dst.fits(n_frames, Bound32::Pitch) || src_row_stride % 2 != 0 ||
      reinterpret_cast<uintptr_t>(d_src) % 2 != 0 || (n_frames > 1 && src_frame_stride % 2 != 0))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad row / frame stride or alignment (source rows hold %d uint16 samples)", width);
  if (overlaps(src, dst, n_frames)) return fail(ctx, D2PC_ERR_INVALID_ARG, "source and destination overlap");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const MedianArgs m = median_args(ctx, width, height, n_frames, src_row_stride, src.kernel_frame_stride(n_frames),
                                   dst_row_stride, dst.kernel_frame_stride(n_frames));
  D2PC_HIP(ctx, launch_mono16_to_mono8(d_src, d_dst, m, static_cast<hipStream_t>(stream)));
  return D2PC_OK;
}

static int median_device(d2pc_ctx *ctx, const void *d_src, int width, int height, size_t src_row_stride,
                         size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_row_stride,
                         size_t dst_frame_stride, int ksize, void *stream, bool roi_only) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d_src || !d_dst || d_src == d_dst) return fail(ctx, D2PC_ERR_INVALID_ARG, "bad device pointers");
  if (int st = check_median(ctx, true, ksize)) return st;
  if (width <= 0 || height <= 0 || n_frames <= 0 || n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", width, height, n_frames);
  const Plane src{d_src, src_row_stride, src_frame_stride, size_t(width), height};
  const Plane dst{d_dst, dst_row_stride, dst_frame_stride, size_t(width), height};
  if (!src.fits(n_frames, Bound32::Pitch, FrameRule::WholeRows) || !dst.fits(n_frames, Bound32::Pitch, FrameRule::WholeRows))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "row stride smaller than the width, or frame stride smaller than a frame's rows");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  MedianArgs m = median_args(ctx, width, height, n_frames, src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride);
  if (roi_only) {
    const int b = ctx->cfg.border;
    if (width <= 2 * b || height <= 2 * b) return D2PC_OK;  // empty ROI: nothing is read downstream
    m.out_x0 = m.out_y0 = uint32_t(b);
    m.out_w = uint32_t(width - 2 * b);
    m.out_h = uint32_t(height - 2 * b);
  }
  D2PC_HIP(ctx, launch_median(d_src, d_dst, m, ksize, static_cast<hipStream_t>(stream)));
  return D2PC_OK;
}

int d2pc_median_device(d2pc_ctx *ctx, const void *d_src, int width, int height, size_t src_row_stride,
                       size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_row_stride,
                       size_t dst_frame_stride, int ksize, void *stream) {
  return median_device(ctx, d_src, width, height, src_row_stride, src_frame_stride, n_frames, d_dst, dst_row_stride,
                       dst_frame_stride, ksize, stream, false);
}

int d2pc_median_roi_device(d2pc_ctx *ctx, const void *d_src, int width, int height, size_t src_row_stride,
                           size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_row_stride,
                           size_t dst_frame_stride, int ksize, void *stream) {
  return median_device(ctx, d_src, width, height, src_row_stride, src_frame_stride, n_frames, d_dst, dst_row_stride,
                       dst_frame_stride, ksize, stream, true);
}

}  // extern "C"

// ---- Device-resident callback body for a batch: (rescale ->) median(ROI) -> reproject, in order on the caller's stream ----
// Filter and points tile by tile in one kernel; the filtered frames never reach memory.  `g` describes the 8-bit frames
// at `src`; `m` is their filter with the ROI as its output rectangle.
static int enqueue_one_kernel(d2pc_ctx *ctx, const Geom &g, const void *src, const MedianArgs &m, int ksize, void *d_out,
                              uint32_t *d_idx, uint32_t *d_counts, hipStream_t stream) {
  LaunchArgs a;
  a.out_points = d_out;
  a.out_index = d_idx;
  a.counts = d_counts;
  a.dtype = D2PC_DTYPE_U8;
  a.stream = stream;
  a.geom = g;
  if (int st = fill_q(ctx, a, int(g.width))) return st;
  a.qs.w_safe = w_safe_for(ctx, g);
  // (the COMPACT form hands row counts over between the tiles of a band: its own state, its frames in resident sub-batches)
  if (ctx->cfg.mode == D2PC_MODE_COMPACT) return enqueue_callback_compact(ctx, a, m, src, ksize);
  D2PC_HIP(ctx, launch_callback_bs(a, m, src, ksize));
  return D2PC_OK;
}

extern "C" int d2pc_process_mono_device(d2pc_ctx *ctx, const void *d_image, int dtype, int width, int height,
                                        size_t row_stride, size_t frame_stride, int n_frames, int median_ksize,
                                        float scale, void *d_out, uint32_t *d_idx, size_t out_frame_stride,
                                        uint32_t *d_counts, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d_image || !d_out) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  if (!ctx->have_q) return fail(ctx, D2PC_ERR_NOT_CALIBRATED, "Q matrix not set");
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return fail(ctx, D2PC_ERR_INVALID_ARG, "d_out_points must be 16-byte aligned");
  const bool bridge16 = dtype == D2PC_DTYPE_MONO16;
  if (dtype != D2PC_DTYPE_U8 && !bridge16) return fail(ctx, D2PC_ERR_BAD_DTYPE, "dtype %d is not U8 / MONO16", dtype);
  const bool median = median_ksize > 1;
  int st;
  if (median && (st = check_median(ctx, true, median_ksize)) != D2PC_OK) return st;
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const bool compact = ctx->cfg.mode == D2PC_MODE_COMPACT;
  const int pxt = compact ? ctx->pxt_compact : parity_pxt(ctx, width, height, n_frames, D2PC_DTYPE_U8);  // (the reprojection sees 8-bit frames)
  Geom gin;  // validates the caller's layout
  st = make_geom(ctx, bridge16 ? int(D2PC_DTYPE_U16) : int(D2PC_DTYPE_U8), scale, width, height, row_stride, frame_stride,
                 n_frames, out_frame_stride, pxt, &gin);
  if (st != D2PC_OK) return st;
  if (bridge16 && reinterpret_cast<uintptr_t>(d_image) % 2 != 0) return fail(ctx, D2PC_ERR_INVALID_ARG, "d_image is not 2-byte aligned");
  hipStream_t user = static_cast<hipStream_t>(stream);
  if (gin.roi_n == 0) {
    if (d_counts) D2PC_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * size_t(n_frames), user));
    return D2PC_OK;
  }
  if (compact && !d_counts) return fail(ctx, D2PC_ERR_INVALID_ARG, "COMPACT mode needs a d_counts buffer");
  const size_t kpitch = (size_t(width) + 255) & ~size_t(255), kframe = kpitch * size_t(height);  // scratch: 8-bit frames on a 256-byte pitch
  // filter + points in one kernel, which needs no filtered frames?  (d2pc_route.hpp)
  CallbackCall call{};
  call.width = width;
  call.height = height;
  call.n_frames = n_frames;
  call.median = median;
  call.bridge16 = bridge16;
  call.captured = capture_info(user, nullptr);
  call.compact = compact;
  call.roi_w = gin.roi_w;
  MedianArgs roi_filter = median_args(ctx, width, height, n_frames, kpitch, kframe, kpitch, kframe);  // (as launched over 8-bit scratch frames)
  median_roi_only(roi_filter, gin, height);
  call.bs_median = median && median_uses_bs(roi_filter, median_ksize);
  const CallbackPlan plan = plan_callback(CallbackTuning{ctx->cb_chunks, ctx->cb_fused, ctx->cb_fused_compact}, call);
  // The filtered (and rescaled) frames of the two-launch form live in a scratch buffer that belongs to THIS stream's
  // work: like the compaction state, one per stream in flight, so that double-buffered use of a context on two
  // streams never overwrites another call's filtered frames (advisor, round 2).  A capture takes an existing idle
  // one (d2pc_reserve_mono, or a call of this size made earlier) and keeps it.
  const size_t need_med = median && !plan.one_kernel ? kframe * size_t(n_frames) : 0;
  const size_t need_cvt = bridge16 ? kframe * size_t(n_frames) : 0;
  StateBuf *scratch = nullptr;
  if ((need_med || need_cvt) && (st = acquire_buf(ctx, ctx->cb_scratch, user, need_med, need_cvt, nullptr, &scratch)) != D2PC_OK) return st;
  void *const d_med = scratch ? scratch->p : nullptr;
  void *const d_cvt = scratch ? scratch->p2 : nullptr;
  Frames k{d_image, row_stride, frame_stride};
  Geom g;  // the 8-bit frames the reprojection reads
  if (plan.overlap) {
#if D2PC_EXPERIMENTS  // (the product's plan is fed one chunk and never answers `overlap`)
    st = process_mono_overlap_lab(ctx, k, width, height, n_frames, plan.chunk, bridge16, median_ksize, d_cvt, d_med, kpitch,
                                  kframe, gin, scale, pxt, d_out, d_idx, out_frame_stride, d_counts, user);
#endif
  } else if ((st = prepare_mono(ctx, &k, width, height, n_frames, bridge16, plan.one_kernel ? 0 : median_ksize, d_cvt, d_med,
                                kpitch, kframe, gin, user)) == D2PC_OK &&  // (one kernel: the rescale alone runs in front of it)
             (st = make_geom(ctx, D2PC_DTYPE_U8, scale, width, height, k.pitch, k.frame, n_frames, out_frame_stride, pxt, &g)) == D2PC_OK) {
    if (!plan.one_kernel) {
      st = enqueue(ctx, g, k.p, D2PC_DTYPE_U8, d_out, d_idx, d_counts, user);
    } else {
      roi_filter.src_row_stride = uint32_t(k.pitch);  // (the filter now reads where the kernel does)
      roi_filter.src_frame_stride = k.frame;
      st = enqueue_one_kernel(ctx, g, k.p, roi_filter, median_ksize, d_out, d_idx, d_counts, user);
    }
  }
  if (st != D2PC_OK) return st;
  if (scratch && !scratch->captured) scratch->dirty = true;  // (inside a capture the record would become a graph node; the buffer is the graph's)
  return D2PC_OK;
}
