// d2pc_capi_mono.hip -- what happens to a mono image before the reprojection, on the device (reference cpp:50-61):
// cv_bridge's mono16 rescale, cv::medianBlur, and the whole callback body for a resident batch (d2pc_process_mono_device).
#include "d2pc_ctx.hpp"

using namespace d2pc;
using namespace d2pc::host;

namespace d2pc {
namespace host {

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
  MedianArgs m;
  m.algo = ctx->median_algo;
  m.width = uint32_t(width);
  m.height = uint32_t(height);
  m.n_frames = uint32_t(n_frames);
  m.src_row_stride = uint32_t(src_row_stride);
  m.dst_row_stride = uint32_t(dst_row_stride);
  m.src_frame_stride = src.kernel_frame_stride(n_frames);
  m.dst_frame_stride = dst.kernel_frame_stride(n_frames);
  D2PC_HIP(ctx, launch_mono16_to_mono8(d_src, d_dst, m, static_cast<hipStream_t>(stream)));
  return D2PC_OK;
}

static int median_device(d2pc_ctx *ctx, const void *d_src, int width, int height, size_t src_row_stride,
                         size_t src_frame_stride, int n_frames, void *d_dst, size_t dst_row_stride,
                         size_t dst_frame_stride, int ksize, void *stream, bool roi_only) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d_src || !d_dst || d_src == d_dst) return fail(ctx, D2PC_ERR_INVALID_ARG, "bad device pointers");
  if (!median_ksize_supported(ksize)) return fail(ctx, D2PC_ERR_INVALID_ARG, "ksize %d not in {3,5,7,9,11}", ksize);
  if (width <= 0 || height <= 0 || n_frames <= 0 || n_frames > 65535)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "bad size %dx%d x%d", width, height, n_frames);
  const Plane src{d_src, src_row_stride, src_frame_stride, size_t(width), height};
  const Plane dst{d_dst, dst_row_stride, dst_frame_stride, size_t(width), height};
  if (!src.fits(n_frames, Bound32::Pitch, FrameRule::WholeRows) || !dst.fits(n_frames, Bound32::Pitch, FrameRule::WholeRows))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "row stride smaller than the width, or frame stride smaller than a frame's rows");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  MedianArgs m;
  m.algo = ctx->median_algo;
  m.width = uint32_t(width);
  m.height = uint32_t(height);
  m.n_frames = uint32_t(n_frames);
  m.src_row_stride = uint32_t(src_row_stride);
  m.dst_row_stride = uint32_t(dst_row_stride);
  m.src_frame_stride = src_frame_stride;
  m.dst_frame_stride = dst_frame_stride;
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

// ---------------------------------------------------------------------------
// Device-resident callback body for a batch: (rescale ->) median(ROI) -> reproject, the VALU-bound filter of
// one half of the batch overlapped with the HBM-bound reprojection of the other on two streams.
// ---------------------------------------------------------------------------
namespace {

// The filter stream and the reprojection stream (plain streams: see the header for why not CU-masked ones).
int callback_streams(d2pc_ctx *ctx) {
  if (!ctx->cb_stream_m) D2PC_HIP(ctx, hipStreamCreateWithFlags(&ctx->cb_stream_m, hipStreamNonBlocking));
  if (!ctx->cb_stream_r) D2PC_HIP(ctx, hipStreamCreateWithFlags(&ctx->cb_stream_r, hipStreamNonBlocking));
  return D2PC_OK;
}

int callback_event(d2pc_ctx *ctx, size_t i, hipEvent_t *e) {
  while (ctx->cb_events.size() <= i) {
    hipEvent_t ev;
    D2PC_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ctx->cb_events.push_back(ev);
  }
  *e = ctx->cb_events[i];
  return D2PC_OK;
}

}  // namespace

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
  if (median && !median_ksize_supported(median_ksize))
    return fail(ctx, D2PC_ERR_INVALID_ARG, "median ksize %d not in {3,5,7,9,11}", median_ksize);
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const bool compact = ctx->cfg.mode == D2PC_MODE_COMPACT;
  const int pxt = compact ? ctx->pxt_compact : parity_pxt(ctx, width, height, n_frames, D2PC_DTYPE_U8);  // (the reprojection sees 8-bit frames)
  Geom gin;  // validates the caller's layout
  int st = make_geom(ctx, bridge16 ? int(D2PC_DTYPE_U16) : int(D2PC_DTYPE_U8), scale, width, height, row_stride,
                     frame_stride, n_frames, out_frame_stride, pxt, &gin);
  if (st != D2PC_OK) return st;
  if (bridge16 && reinterpret_cast<uintptr_t>(d_image) % 2 != 0) return fail(ctx, D2PC_ERR_INVALID_ARG, "d_image is not 2-byte aligned");
  hipStream_t user = static_cast<hipStream_t>(stream);
  if (gin.roi_n == 0) {
    if (d_counts) D2PC_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * size_t(n_frames), user));
    return D2PC_OK;
  }
  if (compact && !d_counts) return fail(ctx, D2PC_ERR_INVALID_ARG, "COMPACT mode needs a d_counts buffer");
  const bool capturing = capture_info(user, nullptr);
  // scratch: the 8-bit frames on a 256-byte pitch
  const size_t kpitch = (size_t(width) + 255) & ~size_t(255), kframe = kpitch * size_t(height);
  // chunked overlap?  filter + points in one kernel, which needs no filtered frames?  (d2pc_route.hpp)
  CallbackCall call{};
  call.width = width;
  call.height = height;
  call.n_frames = n_frames;
  call.median = median;
  call.bridge16 = bridge16;
  call.captured = capturing;
  call.compact = compact;
  call.roi_w = gin.roi_w;
  if (median) {
    MedianArgs probe;
    probe.algo = ctx->median_algo;
    probe.n_frames = uint32_t(n_frames);
    median_roi_only(probe, gin, height);
    call.bs_median = median_uses_bs(probe, median_ksize);
  }
  const CallbackPlan plan = plan_callback(CallbackTuning{ctx->cb_chunks, ctx->cb_fused, ctx->cb_fused_compact}, call);
  const bool one_kernel = plan.one_kernel, overlap = plan.overlap;
  const int chunk = plan.chunk;
  // The filtered (and rescaled) frames of the two-launch form live in a scratch buffer that belongs to THIS stream's
  // work: like the compaction state, one per stream in flight, so that double-buffered use of a context on two
  // streams never overwrites another call's filtered frames (advisor, round 2).  A capture takes an existing idle
  // one (d2pc_reserve_mono, or a call of this size made earlier) and keeps it.
  const size_t need_med = median && !one_kernel ? kframe * size_t(n_frames) : 0;
  const size_t need_cvt = bridge16 ? kframe * size_t(n_frames) : 0;
  StateBuf *scratch = nullptr;
  if (need_med || need_cvt) {
    if ((st = acquire_buf(ctx, ctx->cb_scratch, user, need_med, need_cvt, nullptr, &scratch)) != D2PC_OK) return st;
  }
  void *const d_cb_med = scratch ? scratch->p : nullptr;
  void *const d_cb_cvt = scratch ? scratch->p2 : nullptr;
  hipStream_t sm = user, sr = user;
  if (overlap) {
    if ((st = callback_streams(ctx)) != D2PC_OK) return st;
    // the two internal streams and their events are ONE set per context: a second overlapped call (from any
    // stream) is ordered behind the previous one
    if (!ctx->cb_overlap_done) D2PC_HIP(ctx, hipEventCreateWithFlags(&ctx->cb_overlap_done, hipEventDisableTiming));
    if (ctx->cb_overlap_pending) D2PC_HIP(ctx, hipStreamWaitEvent(user, ctx->cb_overlap_done, 0));
    sm = ctx->cb_stream_m;
    sr = ctx->cb_stream_r;
    hipEvent_t fork;
    if ((st = callback_event(ctx, 0, &fork)) != D2PC_OK) return st;
    D2PC_HIP(ctx, hipEventRecord(fork, user));
    D2PC_HIP(ctx, hipStreamWaitEvent(sm, fork, 0));
    D2PC_HIP(ctx, hipStreamWaitEvent(sr, fork, 0));
  }
  size_t ev = 1;
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int nf = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    const uint8_t *src = static_cast<const uint8_t *>(d_image) + size_t(f0) * frame_stride;
    const void *kin = src;
    size_t kin_pitch = row_stride, kin_frame = frame_stride;
    MedianArgs m;
    m.algo = ctx->median_algo;
    m.width = uint32_t(width);
    m.height = uint32_t(height);
    m.n_frames = uint32_t(nf);
    if (bridge16) {
      m.src_row_stride = uint32_t(row_stride);
      m.dst_row_stride = uint32_t(kpitch);
      m.src_frame_stride = frame_stride;
      m.dst_frame_stride = kframe;
      uint8_t *dst = static_cast<uint8_t *>(d_cb_cvt) + size_t(f0) * kframe;
      D2PC_HIP(ctx, launch_mono16_to_mono8(src, dst, m, sm));
      kin = dst;
      kin_pitch = kpitch;
      kin_frame = kframe;
    }
    if (median) {
      m.src_row_stride = uint32_t(kin_pitch);
      m.dst_row_stride = uint32_t(kpitch);
      m.src_frame_stride = kin_frame;
      m.dst_frame_stride = kframe;
      median_roi_only(m, gin, height);
      if (one_kernel) {
        // filter and points tile by tile in one kernel; the filtered frames never reach memory
        Geom g;
        if ((st = make_geom(ctx, D2PC_DTYPE_U8, scale, width, height, kin_pitch, kin_frame, nf, out_frame_stride, pxt, &g)) != D2PC_OK)
          return st;
        LaunchArgs a;
        a.out_points = static_cast<uint8_t *>(d_out) + size_t(f0) * out_frame_stride * 16;
        a.out_index = d_idx ? d_idx + size_t(f0) * out_frame_stride : nullptr;
        a.counts = d_counts ? d_counts + f0 : nullptr;
        a.dtype = D2PC_DTYPE_U8;
        a.stream = sr;
        if ((st = fill_q(ctx, a, width)) != D2PC_OK) return st;
        a.qs.w_safe = w_safe_for(ctx, g);
        if (compact) {  // the COMPACT form hands row counts over between the tiles of a band: its own state
          // Residency: sub-batches of at most cc.nfc frames, launched back to back on the same stream (d2pc_route.hpp)
          const uint32_t tiles_x = cb_tiles_x(g.roi_w), tiles_y = cb_tiles_y(g.roi_n / g.roi_w);  // (ROI rows)
          const CallbackCompactPlan cc =
              plan_callback_compact(ctx->cu_count, ctx->cb_pipe_blocks_per_cu, ctx->cb_fused_compact, tiles_x, tiles_y, uint32_t(nf));
          const uint32_t nfc = cc.nfc;
          for (int s0 = 0; s0 < nf; s0 += int(nfc)) {
            const int ns = nf - s0 < int(nfc) ? nf - s0 : int(nfc);
            Geom gs;
            if ((st = make_geom(ctx, D2PC_DTYPE_U8, scale, width, height, kin_pitch, kin_frame, ns, out_frame_stride, pxt, &gs)) != D2PC_OK)
              return st;
            LaunchArgs as = a;
            as.keep_timeout = s0 > 0;  // one flag for the whole call: a later sub-batch's state clear must not wipe an earlier one's give-up
            MedianArgs ms = m;
            ms.n_frames = uint32_t(ns);
            as.out_points = static_cast<uint8_t *>(a.out_points) + size_t(s0) * out_frame_stride * 16;
            as.out_index = a.out_index ? a.out_index + size_t(s0) * out_frame_stride : nullptr;
            as.counts = a.counts + s0;
            uint32_t stride = 0;
            as.state_bytes = callback_compact_state_bytes(tiles_x, tiles_y, uint32_t(ns), &stride);
            gs.frame_state_stride = stride;
            as.stats = ctx->d_stats;
            StateBuf *sb = nullptr;
            if ((st = acquire_buf(ctx, ctx->states, sr, as.state_bytes, 0, nullptr, &sb)) != D2PC_OK) return st;
            as.state = sb->p;
            sb->algo = 2;  // its header carries the hand-off's timeout flag, like the single pass's
            sb->pp_clean = false;
            sb->hdr_off = 0;
            as.geom = gs;
            as.compact_algo = 1;
            const CallbackCompactPlan::Sub sub = cc.sub(uint32_t(ns));
            if (sub.pipelined) {  // (the one-tile-per-block form takes its grid from the launch's own tiles)
              as.grid = sub.grid;
              as.compact_algo = 2;
            }
            D2PC_HIP(ctx, launch_callback_bs_compact(as, ms, static_cast<const uint8_t *>(kin) + size_t(s0) * kin_frame, median_ksize));
            if (!sb->captured) sb->dirty = true;
          }
          continue;
        }
        a.geom = g;
        D2PC_HIP(ctx, launch_callback_bs(a, m, kin, median_ksize));
        continue;
      }
      uint8_t *dst = static_cast<uint8_t *>(d_cb_med) + size_t(f0) * kframe;
      D2PC_HIP(ctx, launch_median(kin, dst, m, median_ksize, sm));
      kin = dst;
      kin_pitch = kpitch;
      kin_frame = kframe;
    }
    if (overlap) {
      hipEvent_t done;
      if ((st = callback_event(ctx, ev++, &done)) != D2PC_OK) return st;
      D2PC_HIP(ctx, hipEventRecord(done, sm));
      D2PC_HIP(ctx, hipStreamWaitEvent(sr, done, 0));
    }
    Geom g;
    if ((st = make_geom(ctx, D2PC_DTYPE_U8, scale, width, height, kin_pitch, kin_frame, nf, out_frame_stride, pxt, &g)) != D2PC_OK)
      return st;
    st = enqueue(ctx, g, kin, D2PC_DTYPE_U8, static_cast<uint8_t *>(d_out) + size_t(f0) * out_frame_stride * 16,
                 d_idx ? d_idx + size_t(f0) * out_frame_stride : nullptr, d_counts ? d_counts + f0 : nullptr, sr);
    if (st != D2PC_OK) return st;
  }
  if (overlap) {
    hipEvent_t join;
    if ((st = callback_event(ctx, ev++, &join)) != D2PC_OK) return st;
    D2PC_HIP(ctx, hipEventRecord(join, sr));  // every filter launch is ordered before a reprojection on sr
    D2PC_HIP(ctx, hipStreamWaitEvent(user, join, 0));
    D2PC_HIP(ctx, hipEventRecord(ctx->cb_overlap_done, user));
    ctx->cb_overlap_pending = true;
  }
  if (scratch && !scratch->captured) {  // (inside a capture the record would become a graph node; the buffer is the graph's)
    scratch->dirty = true;
  }
  return D2PC_OK;
}
