// lab/d2pc_capi_mono_overlap.hip -- closed experiment, host code only: d2pc_process_mono_device's two-launch form cut into
// `callback_chunks` chunks, the VALU-bound filter of one chunk on one internal stream beside the HBM-bound reprojection of
// another on a second one.  It did not pay reliably (profiles/r02_callback_overlap.txt: 4K x16 8-10 % slower, 752x480 x64
// 2 % faster), so the product serves the batch in order on the caller's stream and only the experiment build compiles this.
#include "../d2pc_ctx.hpp"

using namespace d2pc;
using namespace d2pc::host;

static int callback_event(d2pc_ctx *ctx, size_t i, hipEvent_t *e) {
  while (ctx->cb_events.size() <= i) {
    hipEvent_t ev;
    D2PC_HIP(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    ctx->cb_events.push_back(ev);
  }
  *e = ctx->cb_events[i];
  return D2PC_OK;
}

namespace d2pc {
namespace host {

int process_mono_overlap_lab(d2pc_ctx *ctx, Frames in, int width, int height, int n_frames, int chunk, bool rescale, int ksize,
                             void *d_cvt, void *d_med, size_t kpitch, size_t kframe, const Geom &roi, float scale, int pxt,
                             void *d_out, uint32_t *d_idx, size_t out_frame_stride, uint32_t *d_counts, hipStream_t user) {
  int st;
  // the filter stream and the reprojection stream (plain streams, not CU-masked ones)
  if (!ctx->cb_stream_m) D2PC_HIP(ctx, hipStreamCreateWithFlags(&ctx->cb_stream_m, hipStreamNonBlocking));
  if (!ctx->cb_stream_r) D2PC_HIP(ctx, hipStreamCreateWithFlags(&ctx->cb_stream_r, hipStreamNonBlocking));
  // the two internal streams and their events are ONE set per context: a second overlapped call (from any
  // stream) is ordered behind the previous one
  if (!ctx->cb_overlap_done) D2PC_HIP(ctx, hipEventCreateWithFlags(&ctx->cb_overlap_done, hipEventDisableTiming));
  if (ctx->cb_overlap_pending) D2PC_HIP(ctx, hipStreamWaitEvent(user, ctx->cb_overlap_done, 0));
  const hipStream_t sm = ctx->cb_stream_m, sr = ctx->cb_stream_r;
  hipEvent_t fork;
  if ((st = callback_event(ctx, 0, &fork)) != D2PC_OK) return st;
  D2PC_HIP(ctx, hipEventRecord(fork, user));
  D2PC_HIP(ctx, hipStreamWaitEvent(sm, fork, 0));
  D2PC_HIP(ctx, hipStreamWaitEvent(sr, fork, 0));
  size_t ev = 1;
  for (int f0 = 0; f0 < n_frames; f0 += chunk) {
    const int nf = n_frames - f0 < chunk ? n_frames - f0 : chunk;
    Frames k{static_cast<const uint8_t *>(in.p) + size_t(f0) * in.frame, in.pitch, in.frame};
    st = prepare_mono(ctx, &k, width, height, nf, rescale, ksize, d_cvt ? static_cast<uint8_t *>(d_cvt) + size_t(f0) * kframe : nullptr,
                      d_med ? static_cast<uint8_t *>(d_med) + size_t(f0) * kframe : nullptr, kpitch, kframe, roi, sm);
    if (st != D2PC_OK) return st;
    hipEvent_t done;
    if ((st = callback_event(ctx, ev++, &done)) != D2PC_OK) return st;
    D2PC_HIP(ctx, hipEventRecord(done, sm));
    D2PC_HIP(ctx, hipStreamWaitEvent(sr, done, 0));
    Geom g;
    if ((st = make_geom(ctx, D2PC_DTYPE_U8, scale, width, height, k.pitch, k.frame, nf, out_frame_stride, pxt, &g)) != D2PC_OK) return st;
    st = enqueue(ctx, g, k.p, D2PC_DTYPE_U8, static_cast<uint8_t *>(d_out) + size_t(f0) * out_frame_stride * 16,
                 d_idx ? d_idx + size_t(f0) * out_frame_stride : nullptr, d_counts ? d_counts + f0 : nullptr, sr);
    if (st != D2PC_OK) return st;
  }
  hipEvent_t join;
  if ((st = callback_event(ctx, ev++, &join)) != D2PC_OK) return st;
  D2PC_HIP(ctx, hipEventRecord(join, sr));  // every filter launch is ordered before a reprojection on sr
  D2PC_HIP(ctx, hipStreamWaitEvent(user, join, 0));
  D2PC_HIP(ctx, hipEventRecord(ctx->cb_overlap_done, user));
  ctx->cb_overlap_pending = true;
  return D2PC_OK;
}

}  // namespace host
}  // namespace d2pc
