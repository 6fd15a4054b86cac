// d2pc_capi_route.hip -- one device-resident call: launch geometry (make_geom) and the launch itself (enqueue: PARITY one-shot
// blocks; COMPACT two-pass / resident one-launch / single pass, as d2pc_route.hpp's plan_compact chooses), d2pc_process_device.
// The seam it serves: reference src/disparity_to_point_cloud.cpp:60-85.
#include "d2pc_ctx.hpp"

using namespace d2pc;
using namespace d2pc::host;

namespace d2pc {
namespace host {

int grow(d2pc_ctx *ctx, void **p, size_t *cap, size_t need) {
  if (need <= *cap) return D2PC_OK;
  if (*p) {
    D2PC_HIP(ctx, hipFree(*p));
    *p = nullptr;
    *cap = 0;
  }
  size_t want = (need + (size_t(1) << 20) - 1) & ~((size_t(1) << 20) - 1);
  D2PC_HIP(ctx, hipMalloc(p, want));
  *cap = want;
  return D2PC_OK;
}

int parity_pxt(const d2pc_ctx *ctx, int width, int height, int n_frames, int dtype) {
  return parity_pxt(ctx->pxt_parity, dtype == D2PC_DTYPE_F32, ctx->cfg.border, width, height, n_frames);
}

// Validates the frame description and fills the launch geometry.
int make_geom(d2pc_ctx *ctx, int dtype, float scale, int width, int height, size_t row_stride,
              size_t in_frame_stride, int n_frames, size_t out_frame_stride, int pxt, Geom *g) {
  if (dtype != D2PC_DTYPE_F32 && dtype != D2PC_DTYPE_U8 && dtype != D2PC_DTYPE_U16)
    return fail(ctx, D2PC_ERR_BAD_DTYPE, "dtype %d is not F32/U8/U16", dtype);
  if (width <= 0 || height <= 0) return fail(ctx, D2PC_ERR_BAD_SIZE, "bad image size %dx%d", width, height);
  if (uint64_t(width) * uint64_t(height) > (uint64_t(1) << 31))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "image %dx%d exceeds 2^31 pixels", width, height);
  const size_t es = elem_size(dtype);
  if (row_stride < size_t(width) * es || row_stride % es != 0)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "row stride %zu invalid for width %d (elem %zu B)", row_stride, width, es);
  if (n_frames <= 0 || n_frames > 65535) return fail(ctx, D2PC_ERR_BAD_SIZE, "bad frame count %d", n_frames);
  if (n_frames > 1 && (in_frame_stride < size_t(height) * row_stride || in_frame_stride % es != 0))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "input frame stride %zu too small", in_frame_stride);
  // 32-bit byte offsets inside a frame, with room for the tail slots of the
  // last tile (up to 16*256 pixels past the ROI end)
  if ((uint64_t(height) + 4097) * row_stride > 0xffffffffull)
    return fail(ctx, D2PC_ERR_BAD_SIZE, "frame of %d rows x %zu bytes exceeds 32-bit addressing", height, row_stride);
  const int b = ctx->cfg.border;
  memset(g, 0, sizeof *g);
  g->width = uint32_t(width);
  g->border = uint32_t(b);
  g->roi_w = width > 2 * b ? uint32_t(width - 2 * b) : 0u;
  const uint32_t roi_h = height > 2 * b ? uint32_t(height - 2 * b) : 0u;
  if (uint64_t(g->roi_w) * roi_h > (uint64_t(1) << 28))
    return fail(ctx, D2PC_ERR_BAD_SIZE, "ROI of %u x %u exceeds 2^28 points", g->roi_w, roi_h);
  g->roi_n = g->roi_w * roi_h;
  if (n_frames > 1 && out_frame_stride < g->roi_n)
    return fail(ctx, D2PC_ERR_CAPACITY, "output frame stride %zu < %u ROI points", out_frame_stride, g->roi_n);
  g->tiles_per_frame = tiles_of(g->roi_n, pxt);
  g->n_frames = uint32_t(n_frames);
  const uint64_t total = uint64_t(g->tiles_per_frame) * g->n_frames;
  if (total > 0x7fffffffull) return fail(ctx, D2PC_ERR_BAD_SIZE, "batch too large (%llu tiles)", (unsigned long long)total);
  g->total_tiles = uint32_t(total);
  g->groups_per_frame = (g->tiles_per_frame + kGroupTiles - 1) / kGroupTiles;
  g->frame_state_stride = frame_state_stride(g->tiles_per_frame);
  const uint32_t rw = g->roi_w ? g->roi_w : 1u;
  g->s64_v = 64u / rw;
  g->s64_u = 64u % rw;
  g->s832_v = 832u / rw;
  g->s832_u = 832u % rw;
  g->s1024_v = 1024u / rw;
  g->s1024_u = 1024u % rw;
  g->div_roi_w = make_fastdiv(rw);
  g->div_tpf = make_fastdiv(g->tiles_per_frame ? g->tiles_per_frame : 1u);
  g->row_stride = uint32_t(row_stride);
  g->last_off = g->roi_n ? uint32_t((uint64_t(b) + roi_h - 1) * row_stride + (uint64_t(b) + g->roi_w - 1) * es) : 0u;
  g->in_frame_stride = in_frame_stride;
  g->out_frame_stride = out_frame_stride;
  g->scale = scale;
  g->min_disparity = ctx->cfg.min_disparity;
  g->spin_ticks = uint32_t(ctx->spin_timeout_ms) * kSpinTicksPerMs;
  g->pxt = uint32_t(pxt);
  return D2PC_OK;
}

// The same frames cut into tiles of 256 * pxt ROI pixels.
void retile(Geom *g, int pxt) {
  g->tiles_per_frame = tiles_of(g->roi_n, pxt);
  g->total_tiles = uint32_t(uint64_t(g->tiles_per_frame) * g->n_frames);
  g->groups_per_frame = (g->tiles_per_frame + kGroupTiles - 1) / kGroupTiles;
  g->frame_state_stride = frame_state_stride(g->tiles_per_frame);
  g->div_tpf = make_fastdiv(g->tiles_per_frame ? g->tiles_per_frame : 1u);
  g->pxt = uint32_t(pxt);
}

// bound on |u + cx|, |v + cy|, |f| over the frame, scaled by 2^-126: any |W| at least this large keeps every
// quotient below 2^126 < FLT_MAX (QStereo::w_safe: the exact validity predicate of the COMPACT kernels)
double w_safe_for(const d2pc_ctx *ctx, const Geom &g) {
  const double height = double((g.last_off / (g.row_stride ? g.row_stride : 1u)) + 1u);
  const double mx = std::fmax(std::fabs(ctx->qs.cx), std::fabs(ctx->qs.cx + double(g.width)));
  const double my = std::fmax(std::fabs(ctx->qs.cy), std::fabs(ctx->qs.cy + height));
  const double m = std::fmax(std::fabs(ctx->qs.f), std::fmax(mx, my));
  return std::isfinite(m) ? std::ldexp(m, -126) : std::numeric_limits<double>::infinity();
}

// The tuning fields the plans read.
static RouteTuning route_tuning(const d2pc_ctx *ctx) {
  RouteTuning t{};
  t.cu_count = ctx->cu_count;
  t.compact_algo = ctx->cfg.compact_algo;
  t.blocks_per_cu = ctx->blocks_per_cu;
  t.onepass_blocks_per_cu = ctx->onepass_blocks_per_cu;
  t.onepass_form = ctx->onepass_form;
  t.resident_pxt = ctx->resident_pxt;
  t.resident_pair = ctx->resident_pair;
  t.resident_unbounded = ctx->resident_unbounded;
  t.resident_stagger_pct = ctx->resident_stagger_pct;
  t.big_batch_algo = ctx->big_batch_algo;
#if D2PC_EXPERIMENTS
  t.chunk_mb = ctx->chunk_mb;
  t.chunk_first_frames = ctx->chunk_first_frames;
#endif
  return t;
}

// A two-frame call as two one-frame launches (CompactPlan::split).
// Both launches use the stream's one state buffer, with consecutive epochs: the buffer remembers the first of them, so
// d2pc_check_async_error covers the whole CALL (a give-up of frame 0 stores epoch E while the buffer's `epoch` is E + 1).
// A failure of the second enqueue leaves frame 0 launched and counts[0] valid: the call returns the error, the caller's
// stream stays usable (nothing of frame 1 was enqueued), and the output of frame 1 is untouched.
static int enqueue_split(d2pc_ctx *ctx, const Geom &g, const void *d_disp, int dtype, void *d_out, uint32_t *d_idx,
                         uint32_t *d_counts, hipStream_t stream, StateBuf *fixed_state) {
  const uint32_t first = ctx->resident_epoch;
  for (uint32_t f = 0; f < 2u; ++f) {
    Geom g1 = g;
    g1.n_frames = 1;
    g1.total_tiles = g1.tiles_per_frame;
    if (f == 0 && ctx->spin_ticks_first >= 0) g1.spin_ticks = uint32_t(ctx->spin_ticks_first);  // (test hook)
    int st1 = enqueue(ctx, g1, static_cast<const uint8_t *>(d_disp) + uint64_t(f) * g.in_frame_stride, dtype,
                      static_cast<uint8_t *>(d_out) + uint64_t(f) * g.out_frame_stride * 16u,
                      d_idx ? d_idx + uint64_t(f) * g.out_frame_stride : nullptr, d_counts + f, stream, fixed_state, 0, first);
    if (st1 != D2PC_OK) return st1;
  }
  return D2PC_OK;
}

int enqueue(d2pc_ctx *ctx, const Geom &g, const void *d_disp, int dtype, void *d_out, uint32_t *d_idx,
            uint32_t *d_counts, hipStream_t stream, StateBuf *fixed_state, int force_algo, uint32_t call_epoch_first) {
  LaunchArgs a;
  a.disp = d_disp;
  a.out_points = d_out;
  a.out_index = d_idx;
  a.counts = d_counts;
  a.dtype = dtype;
  a.stream = stream;
  a.geom = g;
  a.pxt = int(g.pxt);
  {
    int stq = fill_q(ctx, a, int(g.width));
    if (stq != D2PC_OK) return stq;
  }
  // 16-B row loads need every aligned group of four ROI pixels to sit in one
  // row at a 16-B aligned address
  a.vec_rows = !ctx->no_vec_rows && dtype == D2PC_DTYPE_F32 && g.roi_w % 4 == 0 && g.border % 4 == 0 &&
               g.row_stride % 16 == 0 && g.in_frame_stride % 16 == 0 && reinterpret_cast<uintptr_t>(d_disp) % 16 == 0;
  a.qs.w_safe = w_safe_for(ctx, g);
  if (ctx->cfg.mode == D2PC_MODE_PARITY) {
    a.grid = walk_grid(g.total_tiles, ctx->cu_count, ctx->blocks_per_cu);
    a.parity_small = g.pxt <= 2 || (ctx->parity_small == 1 && g.pxt == 4);
    D2PC_HIP(ctx, launch_parity(a));
    return D2PC_OK;
  }
  if (!d_counts) return fail(ctx, D2PC_ERR_INVALID_ARG, "COMPACT mode needs a d_counts buffer");
  CompactCall call{};
  call.roi_n = g.roi_n;
  call.n_frames = g.n_frames;
  call.pxt = int(g.pxt);
  call.elem_size = int(elem_size(dtype));
  call.is_f32 = dtype == D2PC_DTYPE_F32;
  call.captured = capture_info(stream, nullptr);
  call.force_algo = force_algo;
  const CompactPlan plan = plan_compact(route_tuning(ctx), call);
  if (plan.split) return enqueue_split(ctx, g, d_disp, dtype, d_out, d_idx, d_counts, stream, fixed_state);
  a.compact_algo = plan.algo;
  a.onepass_form = plan.onepass_form;
  a.grid = plan.grid;
  if (plan.pxt != int(g.pxt)) {
    retile(&a.geom, plan.pxt);
    a.pxt = plan.pxt;
  }
  if (plan.lean) a.geom.stagger = plan.stagger;
#if D2PC_EXPERIMENTS
  if (plan.algo == 4) {  // (the chunked two-pass: the product's configuration admits no algorithm 4)
    if (g.roi_n == 0) return fail(ctx, D2PC_ERR_INTERNAL, "empty ROI reached the compaction launch");
    if (uint64_t(a.geom.tiles_per_frame) * a.geom.n_frames > 0x7fffffffull) return fail(ctx, D2PC_ERR_BAD_SIZE, "batch too large");
    uint32_t gw = 0;
    a.geom.frame_state_stride = chunk_frame_state_stride(a.geom.tiles_per_frame, &gw);
    a.chunk_frames = plan.chunk_frames;
    a.chunk_first = plan.chunk_first;
  }
#endif
  if (plan.algo == 3) {
    int ste = take_epoch(ctx, &a.epoch);
    if (ste != D2PC_OK) return ste;
  }
  a.state_bytes = compact_state_bytes(a.geom);
  a.stats = ctx->d_stats;
  StateBuf *sb = nullptr;
  int st = acquire_buf(ctx, ctx->states, stream, state_need(a.state_bytes, plan.self_clean), 0, fixed_state, &sb);
  if (st != D2PC_OK) return st;
  bind_state(*sb, a, plan.self_clean);
#if D2PC_EXPERIMENTS
  if (a.compact_algo == 4) {
    // (tiles per frame, frames): they fix the groups, the padded words and the stride -- two shapes may share a 256-byte-rounded
    // stride and still keep their group totals in different words, and a stale word that is not "empty" would be taken for a total
    const uint64_t sig = (uint64_t(a.geom.tiles_per_frame) << 32) | a.geom.n_frames;
    a.chunk_clear = sb->algo != 4 || sb->chunk_sig != sig;
    sb->chunk_sig = sig;
  }
#endif
  sb->algo = a.compact_algo;
  sb->epoch = a.epoch;
  // (an epoch wrap-around between the two launches of a call starts over below `first`: the range then begins at this launch)
  sb->epoch_first = call_epoch_first && call_epoch_first <= a.epoch ? call_epoch_first : a.epoch;
  const hipError_t launched = launch_compact(a);
  if (launched != hipSuccess) sb->pp_clean = false;  // (nothing ran: the half this launch was to zero for its successor is still dirty)
  D2PC_HIP(ctx, launched);
  if (!sb->captured) sb->dirty = true;  // (a captured buffer is never shared; for the others `done` is recorded when somebody asks)
  return D2PC_OK;
}

// The tile-fused COMPACT callback body (median + points per tile, row counts handed over between the tiles of a band).
// Residency: sub-batches of at most nfc frames, launched back to back on the same stream (d2pc_route.hpp); `a` holds the
// whole call (geometry, outputs, Q), `m` the filter with the ROI as its output rectangle, `src` the 8-bit frames.
int enqueue_callback_compact(d2pc_ctx *ctx, const LaunchArgs &a, const MedianArgs &m, const void *src, int ksize) {
  const Geom &g = a.geom;
  const uint32_t tiles_x = cb_tiles_x(g.roi_w), tiles_y = cb_tiles_y(g.roi_n / g.roi_w);  // (ROI rows)
  const CallbackCompactPlan cc =
      plan_callback_compact(ctx->cu_count, ctx->cb_pipe_blocks_per_cu, ctx->cb_fused_compact, tiles_x, tiles_y, g.n_frames);
  for (uint32_t s0 = 0; s0 < g.n_frames; s0 += cc.nfc) {
    const uint32_t ns = g.n_frames - s0 < cc.nfc ? g.n_frames - s0 : cc.nfc;
    LaunchArgs as = a;
    as.keep_timeout = s0 > 0;  // one flag for the whole call: a later sub-batch's state clear must not wipe an earlier one's give-up
    as.out_points = static_cast<uint8_t *>(a.out_points) + size_t(s0) * g.out_frame_stride * 16;
    as.out_index = a.out_index ? a.out_index + size_t(s0) * g.out_frame_stride : nullptr;
    as.counts = a.counts + s0;
    as.geom.n_frames = ns;
    as.geom.total_tiles = g.tiles_per_frame * ns;
    as.state_bytes = callback_compact_state_bytes(tiles_x, tiles_y, ns, &as.geom.frame_state_stride);
    as.stats = ctx->d_stats;
    MedianArgs ms = m;
    ms.n_frames = ns;
    StateBuf *sb = nullptr;
    int st = acquire_buf(ctx, ctx->states, a.stream, as.state_bytes, 0, nullptr, &sb);
    if (st != D2PC_OK) return st;
    bind_state(*sb, as, false);
    sb->algo = 2;  // its header carries the hand-off's timeout flag, like the single pass's
    const CallbackCompactPlan::Sub sub = cc.sub(ns);
    as.compact_algo = sub.pipelined ? 2 : 1;
    if (sub.pipelined) as.grid = sub.grid;  // (the one-tile-per-block form takes its grid from the launch's own tiles)
    D2PC_HIP(ctx, launch_callback_bs_compact(as, ms, static_cast<const uint8_t *>(src) + size_t(s0) * g.in_frame_stride, ksize));
    if (!sb->captured) sb->dirty = true;
  }
  return D2PC_OK;
}

}  // namespace host
}  // namespace d2pc

extern "C" {

int d2pc_process_device(d2pc_ctx *ctx, const void *d_disp, int dtype, float scale, int width, int height,
                        size_t row_stride, size_t in_frame_stride, int n_frames, void *d_out, uint32_t *d_idx,
                        size_t out_frame_stride, uint32_t *d_counts, void *stream) {
  if (!ctx) return D2PC_ERR_INVALID_ARG;
  if (!d_disp || !d_out) return fail(ctx, D2PC_ERR_INVALID_ARG, "null device pointer");
  if (!ctx->have_q) return fail(ctx, D2PC_ERR_NOT_CALIBRATED, "Q matrix not set");
  if (reinterpret_cast<uintptr_t>(d_out) % 16 != 0) return fail(ctx, D2PC_ERR_INVALID_ARG, "d_out_points must be 16-byte aligned");
  DeviceGuard guard(ctx->device);
  if (!guard.ok) return fail(ctx, D2PC_ERR_NO_DEVICE, "cannot select device %d", ctx->device);
  const bool compact = ctx->cfg.mode == D2PC_MODE_COMPACT;
  Geom g;
  int st = make_geom(ctx, dtype, scale, width, height, row_stride, in_frame_stride, n_frames, out_frame_stride,
                     compact ? ctx->pxt_compact : parity_pxt(ctx, width, height, n_frames, dtype), &g);
  if (st != D2PC_OK) return st;
  if (reinterpret_cast<uintptr_t>(d_disp) % elem_size(dtype) != 0)
    return fail(ctx, D2PC_ERR_INVALID_ARG, "d_disp is not aligned to its sample type");
  hipStream_t s = static_cast<hipStream_t>(stream);  // NULL = HIP's default stream
  if (g.roi_n == 0) {
    if (d_counts) D2PC_HIP(ctx, hipMemsetAsync(d_counts, 0, sizeof(uint32_t) * size_t(n_frames), s));
    return D2PC_OK;
  }
  return enqueue(ctx, g, d_disp, dtype, d_out, d_idx, d_counts, s);
}

}  // extern "C"
